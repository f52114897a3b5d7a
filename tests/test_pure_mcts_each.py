"""oaz_pure_mcts_search_each: one pure-MCTS search per root, each with its own max_playouts, min_node_visits,
exploration_c and rollout stream, and the agent's search_time clock on the device.

CPU: the ABI (struct sizes, symbols, capacities and offsets, every argument check before a device is touched).
GPU: every root's tree byte-equal to the oracle's search of that root alone (c = 0.0 included: its NaN UCT
values must order as the x86 default NaN), uniform parameters byte-equal to oaz_pure_mcts_search, the clock's
deterministic ends and a budget that binds, and Mcts(enforce_search_time=True).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import kat_state, random_positions
from onitama_az import _abi
from onitama_az.pure_mcts import default_config, root_params

SQRT2 = float(np.float32(2.0 ** 0.5))
SEED = 99
# test 1's configuration: the parameters cycle lane by lane (cycle lengths 4, 4 and 5)
G1 = 70
PLAYOUTS = (1, 7, 64, 300)
MIN_VISITS = (0, 1, 5, 8)
CS = (0.0, 0.5, 1.0, SQRT2, 3.0)


def _cfg(playouts, min_visits=5, c=SQRT2, seed=SEED):
    cfg = default_config()
    cfg.max_playouts, cfg.min_node_visits, cfg.exploration_c, cfg.seed = int(playouts), int(min_visits), c, seed
    return cfg


def _mv(m):
    return [int(m[k]) for k in ("from_", "to", "piece", "slot")]


def _lane_params(G):
    g = np.arange(G)
    po = np.array(PLAYOUTS, dtype=np.int32)[g % 4]
    mv = np.array(MIN_VISITS, dtype=np.int32)[g % 4]
    c = np.array(CS, dtype=np.float32)[g % 5]
    streams = np.where(g % 2 == 0, 1000 + 37 * g, (3 << 20) + g).astype(np.uint64)
    return po, mv, c, streams


@pytest.fixture(scope="module")
def mixed(orc):
    """Test 1's roots and parameters with the oracle's answer for every root, computed once."""
    roots = random_positions(orc, G1, seed=83)
    po, mv, c, streams = _lane_params(G1)
    ref = [orc.pure_mcts(_cfg(po[g], mv[g], float(c[g])), int(streams[g]), roots[g])[:3] for g in range(G1)]
    return roots, po, mv, c, streams, ref


def _check_against(r, ref, lanes=None):
    for k, g in enumerate(range(len(ref)) if lanes is None else lanes):
        m, v, nodes = ref[g]
        assert r.tree(k)[: len(nodes)].tobytes() == nodes.tobytes(), g
        assert _mv(r.moves[k]) == _mv(m) and r.values[k] == np.float32(v), g


def _node_count(tree):
    n, i = 1, 0
    while i < n:
        if tree[i]["flags"] & 1:
            n = max(n, int(tree[i]["first"]) + int(tree[i]["nch"]))
        i += 1
    return n


# ---- CPU ------------------------------------------------------------------------------------------------

def test_abi_structs_and_symbols(lib):
    assert C.sizeof(_abi.oaz_pure_mcts_root) == 24 and _abi.oaz_pure_mcts_root.stream.offset == 16
    assert C.sizeof(_abi.oaz_pure_mcts_each_config) == 32 and _abi.PURE_ROOT_DTYPE.itemsize == 24
    assert _abi.oaz_pure_mcts_each_config.search_time_ns.offset == 8
    for name in ("oaz_pure_mcts_each_capacity", "oaz_pure_mcts_search_each"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.oaz_abi_version() == 5


def test_each_capacity_is_the_prefix_sum_of_tree_capacities(lib):
    pairs = [(0, 0), (1, 0), (300, 0), (7, 1), (1600, 8), (0, 5), (64, 5), (5000, 5), (3, 100)]
    par = root_params(len(pairs), [p for p, _ in pairs], [n for _, n in pairs], 1.0, 0)
    caps = [int(lib.oaz_pure_mcts_tree_capacity(C.byref(_cfg(p, n)))) for p, n in pairs]
    assert all(c >= 41 for c in caps)
    off = np.full(len(pairs) + 1, 12345, dtype=np.uintp)
    total = int(lib.oaz_pure_mcts_each_capacity(_abi.ptr(par), len(pairs), _abi.ptr(off)))
    assert total == sum(caps) and [int(x) for x in off] == [sum(caps[:k]) for k in range(len(pairs) + 1)]
    assert int(lib.oaz_pure_mcts_each_capacity(_abi.ptr(par), len(pairs), None)) == total
    assert int(lib.oaz_pure_mcts_each_capacity(_abi.ptr(par), 0, _abi.ptr(off))) == 0 and int(off[0]) == 0


def _raw_call(lib, roots, par, cfg, G=None, tree=None, offsets=None, null=()):
    G = len(roots) if G is None else G
    mv, val = np.zeros(max(G, 1), dtype=_abi.MOVE_DTYPE), np.zeros(max(G, 1), dtype=np.float32)
    po = np.zeros(max(G, 1), dtype=np.int32)
    st = _abi.oaz_pure_mcts_stats()
    st.playouts = 7
    rc = lib.oaz_pure_mcts_search_each(
        None if "roots" in null else _abi.ptr(roots), None if "par" in null else _abi.ptr(par), G,
        None if "cfg" in null else C.byref(cfg), None if "out_move" in null else _abi.ptr(mv),
        None if "out_value" in null else _abi.ptr(val), _abi.ptr(po), C.byref(st),
        None if tree is None else _abi.ptr(tree), None if offsets is None else _abi.ptr(offsets))
    return rc, (lib.oaz_last_error() or b"").decode(), st


def test_argument_checks_come_before_any_device(lib, orc):
    """Every OAZ_ERR_ARG case returns -1 whether or not a GPU is there, and names the root it is about."""
    roots = random_positions(orc, 3, seed=5)

    def cfg(**kw):
        c = _abi.oaz_pure_mcts_each_config()
        c.seed, c.rollout_cap, c.device = 1, 1000, 0
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    good = root_params(3, 10, 1, 1.0, [0, 1, 2])
    for name in ("roots", "par", "cfg", "out_move", "out_value"):
        rc, msg, _ = _raw_call(lib, roots, good, cfg(), null=(name,))
        assert rc == _abi.ERR_ARG and "null" in msg, name
    rc, msg, _ = _raw_call(lib, roots, good, cfg(), G=-1)
    assert rc == _abi.ERR_ARG
    for field, value in (("max_playouts", -1), ("min_node_visits", -3)):
        par = good.copy()
        par[field][1] = value
        rc, msg, _ = _raw_call(lib, roots, par, cfg())
        assert rc == _abi.ERR_ARG and "root 1" in msg and "negative" in msg, (field, msg)
    par = good.copy()
    par["stream"][2] = 1 << 32
    rc, msg, _ = _raw_call(lib, roots, par, cfg())
    assert rc == _abi.ERR_ARG and "root 2" in msg and "stream" in msg, msg
    par["stream"][2] = (1 << 32) - 1  # the largest stream is no argument error (whatever else the call returns)
    rc, msg, _ = _raw_call(lib, roots, par, cfg(rollout_cap=-1))
    assert rc == _abi.ERR_ARG and "rollout_cap" in msg, msg
    rc, msg, _ = _raw_call(lib, roots, good, cfg(search_time_ns=-1))
    assert rc == _abi.ERR_ARG and "search_time_ns" in msg, msg
    for bad in ("to_move", "cards", "squares"):
        # squares: one bit outside the 25 squares (the low 7 bits) in each of the four bitboards in turn
        for board, side, bit in ((None, 0, 0),) if bad != "squares" else (
                ("kings", 0, 0), ("kings", 1, 6), ("pawns", 0, 3), ("pawns", 1, 5)):
            broken = roots.copy()
            if bad == "to_move":
                broken["to_move"][2] = 2
            elif bad == "cards":
                broken["cards"][2][3] = 16
            else:
                broken[board][2][side] |= 1 << bit
            rc, msg, _ = _raw_call(lib, broken, good, cfg())
            assert rc == _abi.ERR_ARG and "root 2 is not a valid state" in msg, (bad, board, side, msg)
    rc, msg, _ = _raw_call(lib, roots, good, cfg(), tree=np.zeros(4096, dtype=_abi.PURE_NODE_DTYPE))
    assert rc == _abi.ERR_ARG and "tree_offsets" in msg, msg


def test_no_roots_is_ok_and_touches_no_device(lib):
    c = _abi.oaz_pure_mcts_each_config()
    c.device = 12345  # never looked at
    rc, _, st = _raw_call(lib, None, None, c, G=0, null=("roots", "par", "out_move", "out_value"))
    assert rc == 0 and st.playouts == 0 and st.max_nodes == 0


# ---- GPU ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_mixed_parameters_in_one_launch_equal_the_oracle(mixed):
    from onitama_az.pure_mcts import pure_mcts_search, pure_mcts_search_each
    roots, po, mv, c, streams, ref = mixed
    r = pure_mcts_search_each(roots, po, mv, c, streams, seed=SEED, with_trees=True)
    _check_against(r, ref)
    assert np.array_equal(r.playouts, po) and r.stats.playouts == int(po.sum())
    # lanes that end unexpanded (max_playouts <= min_node_visits + 1): the pass move, as oaz_pure_mcts_search's
    unexpanded = [g for g in range(G1) if po[g] <= mv[g] + 1]
    assert unexpanded
    for g in unexpanded[:6]:
        one = pure_mcts_search(roots[g:g + 1], int(po[g]), int(mv[g]), float(c[g]), seed=SEED, game_id0=int(streams[g]))
        assert _mv(r.moves[g]) == _mv(one.moves[0]) == [25, 25, 0, 2 * int(roots[g]["to_move"])]
        assert r.values[g] == one.values[0] == 0.0
    for g in (0, 3, 5, 67):  # G = 1
        one = pure_mcts_search_each(roots[g:g + 1], po[g], mv[g], c[g], streams[g], seed=SEED, with_trees=True)
        _check_against(one, ref, lanes=[g])
        assert int(one.playouts[0]) == po[g]


@pytest.mark.gpu
def test_gpu_uniform_parameters_equal_the_existing_entry_point(orc):
    from onitama_az.pure_mcts import pure_mcts_search, pure_mcts_search_each
    roots = random_positions(orc, 24, seed=77)
    for min_visits, c, po in ((5, SQRT2, 300), (1, 1.0, 200)):
        old = pure_mcts_search(roots, po, min_visits, c, seed=SEED, game_id0=1000, with_trees=True)
        new = pure_mcts_search_each(roots, po, min_visits, c, 1000 + np.arange(24), seed=SEED, with_trees=True)
        assert new.moves.tobytes() == old.moves.tobytes() and new.values.tobytes() == old.values.tobytes()
        for g in range(24):
            n = _node_count(old.trees[g])
            assert n > 1 and new.tree(g)[:n].tobytes() == old.trees[g][:n].tobytes(), (g, min_visits)
        assert (new.stats.playouts, new.stats.expansions, new.stats.rollout_plies, new.stats.max_nodes) == (
            old.stats.playouts, old.stats.expansions, old.stats.rollout_plies, old.stats.max_nodes)


@pytest.mark.gpu
def test_gpu_one_wave_and_one_lane_equal_the_existing_entry_point(orc):
    """65 roots: one full wave and one lane in a second block, so both kernels meet their `g >= G` guard and the
    last lane's tree offset (tree 64 of either layout)."""
    from onitama_az.pure_mcts import pure_mcts_search, pure_mcts_search_each
    G, po, min_visits = 65, 60, 1
    roots = random_positions(orc, G, seed=79)
    old = pure_mcts_search(roots, po, min_visits, SQRT2, seed=SEED, game_id0=2000, with_trees=True)
    new = pure_mcts_search_each(roots, po, min_visits, SQRT2, 2000 + np.arange(G), seed=SEED, with_trees=True)
    assert new.moves.tobytes() == old.moves.tobytes() and new.values.tobytes() == old.values.tobytes()
    for g in range(G):
        n = _node_count(old.trees[g])
        assert n > 1 and new.tree(g)[:n].tobytes() == old.trees[g][:n].tobytes(), g
    fields = ("playouts", "expansions", "rollout_plies", "rollout_passes", "rollouts_capped", "max_nodes", "tree_full")
    assert [getattr(new.stats, f) for f in fields] == [getattr(old.stats, f) for f in fields]
    assert new.playouts.tolist() == [po] * G and old.stats.playouts == po * G


@pytest.mark.gpu
def test_gpu_clock_deterministic_ends(orc, mixed):
    from onitama_az.pure_mcts import pure_mcts_search_each
    roots, po, mv, c, streams, ref = mixed
    # a budget that cannot bind: test 1's result (clock off is test 1 itself)
    r = pure_mcts_search_each(roots, po, mv, c, streams, seed=SEED, search_time=10.0, with_trees=True)
    _check_against(r, ref)
    assert np.array_equal(r.playouts, po)
    # 1 ns: exactly min(max_playouts, min_node_visits + 2) playouts
    G = 18
    po2 = np.array((1, 300), dtype=np.int32)[np.arange(G) % 2]
    mv2 = np.array((0, 1, 5), dtype=np.int32)[np.arange(G) % 3]
    r = pure_mcts_search_each(roots[:G], po2, mv2, c[:G], streams[:G], seed=SEED, search_time=1e-9, with_trees=True)
    floor = np.minimum(po2, mv2 + 2)
    assert np.array_equal(r.playouts, floor) and r.stats.playouts == int(floor.sum())
    for g in range(G):
        m, v, nodes, _ = orc.pure_mcts(_cfg(floor[g], mv2[g], float(c[g])), int(streams[g]), roots[g])
        assert r.tree(g)[: len(nodes)].tobytes() == nodes.tobytes(), g
        assert _mv(r.moves[g]) == _mv(m) and r.values[g] == np.float32(v), g


@pytest.mark.gpu
def test_gpu_clock_budget_that_binds(orc, lib):
    """100 000 playouts in 2 ms would be 20 ns per playout of dozens of rollout plies: the clock must cut every
    root, after the floor, and each tree is the oracle's for the playouts the root ran."""
    from onitama_az.pure_mcts import pure_mcts_search_each
    roots = random_positions(orc, 4, seed=41, max_plies=6)
    n, limit = 5, 100_000
    r = pure_mcts_search_each(roots, limit, n, SQRT2, 50 + np.arange(4), seed=SEED, search_time=2e-3, with_trees=True)
    cap = int(lib.oaz_pure_mcts_tree_capacity(C.byref(_cfg(limit, n))))
    assert [int(x) for x in r.offsets] == [cap * k for k in range(5)]
    print("playouts run in 2 ms:", r.playouts.tolist())
    for g in range(4):
        ran = int(r.playouts[g])
        assert n + 2 <= ran < limit, (g, ran)
        m, v, nodes, _ = orc.pure_mcts(_cfg(ran, n), 50 + g, roots[g], cap=cap)
        assert r.tree(g)[: len(nodes)].tobytes() == nodes.tobytes(), g
        assert _mv(r.moves[g]) == _mv(m) and r.values[g] == np.float32(v), g


@pytest.mark.gpu
def test_gpu_mcts_agent_with_the_clock_equals_mcts(kats):
    from onitama_az.pure_mcts import Mcts
    from test_pure_mcts import TACTIC_PARAMS
    for case in kats["tactics"]:
        mv, c, po = TACTIC_PARAMS[case["src"].split()[-1]]
        root = kat_state(case["state"], case["color"])
        plain = Mcts(min_node_visits=mv, exploration_c=c, max_playouts=po, seed=5)
        timed = Mcts(search_time=10.0, min_node_visits=mv, exploration_c=c, max_playouts=po, seed=5,
                     enforce_search_time=True)
        assert timed.id() == Mcts(search_time=10.0, min_node_visits=mv, exploration_c=c, max_playouts=po).id()
        for _ in range(2):  # the same call count: the same streams
            a, b = plain._search(root), timed._search(root)
            assert a.moves.tobytes() == b.moves.tobytes() and a.values.tobytes() == b.values.tobytes()
            assert int(b.playouts[0]) == po
        assert _mv(b.moves[0]) == case["expected"], case["src"]
