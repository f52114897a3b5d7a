"""GPU: the leaf-parallel search (oaz_config.leaf_batch, csrc/oaz_search_par.hip) against the Python statement
of its rule (tests/leaf_batch_ref.py): every dumped tree index for index, pi, the move and the round statistics,
with the HASH evaluator (every value exact in fp32) and with the trained 3-block network (the reference's
evaluator then calls the GPU network once per leaf); the search_time budget; and every refusal."""
import math

import numpy as np
import pytest

import leaf_batch_ref as lbr
from leaf_batch_util import (assert_tree_equals, kat_root, midgame_roots, ref_search, sparse_endgame, start_root)
from onitama_az import _abi
from onitama_az.engine import Engine

pytestmark = pytest.mark.gpu

LS = (1, 2, 7, 16)


def _mv(m):
    return tuple(int(m[k]) for k in ("from_", "to", "piece", "slot"))


@pytest.fixture(scope="module")
def root_sets(orc, kats):
    """The calls of one case: each entry is the roots of one oaz_search."""
    return [
        start_root(orc, 0),
        start_root(orc, 1),
        midgame_roots(orc, 3),                                # three roots in one call
        sparse_endgame(0),                                    # won leaves repeat within a round
        kat_root(kats, "blue_to_move_no_legal_moves", 1),     # state.rs:818-850 (one of Blue's cards has no move)
        kat_root(kats, "no_legal_moves_at_all", 1),           # state.rs:852-889: the root expands to no children
    ]


_REF = {}


def _ref(root, sims, c, L):
    """The Python rule's answer, computed once per (root, sims, c, L) and shared."""
    key = (root.tobytes(), sims, c, L)
    if key not in _REF:
        _REF[key] = ref_search(root, sims, c, L)
    return _REF[key]


def _check_search(e, roots, sims, c, L, evaluator=None):
    r = e.search(roots)
    G = len(roots)
    want = [ref_search(roots[g], sims, c, L, evaluator) if evaluator else _ref(roots[g], sims, c, L) for g in range(G)]
    for g, (mv, pi, nodes, _) in enumerate(want):
        assert_tree_equals(e.tree(g), nodes)
        assert np.array_equal(r.pi[g].reshape(-1), pi) and _mv(r.moves[g]) == mv, g
    rounds, disc = (sum(w[3][k] for w in want) for k in (0, 1))
    assert e.leaf_batch_stats() == (rounds, sims * G, disc)
    assert r.stats.sims == sims * G and np.array_equal(e.search_playouts(G), np.full(G, sims))
    return r


@pytest.mark.parametrize("c", [5.0, math.sqrt(2.0)], ids=["c5", "csqrt2"])
@pytest.mark.parametrize("sims_of", [lambda L: 1, lambda L: 2, lambda L: L + 1, lambda L: 3 * L + 5, lambda L: 400],
                         ids=["1", "2", "L+1", "3L+5", "400"])
@pytest.mark.parametrize("L", LS)
def test_hash_trees_equal_the_rule(root_sets, L, sims_of, c):
    sims = sims_of(L)
    with Engine(games=3, sims=sims, c_puct=c, train_noise=0, evaluator=_abi.EVAL_HASH, blocks=0, leaf_batch=L) as e:
        for roots in root_sets:
            _check_search(e, roots, sims, c, L)


@pytest.mark.parametrize("evaluator", ["hash", "nn"])
def test_leaf_batch_one_is_leaf_batch_zero(orc, trained3, evaluator):
    """leaf_batch = 1 dumps what leaf_batch = 0 (k_search_lat) dumps on the same engine configuration."""
    roots = midgame_roots(orc, 3)
    kw = (dict(evaluator=_abi.EVAL_HASH, blocks=0) if evaluator == "hash" else
          dict(evaluator=_abi.EVAL_NN, blocks=3, precision=_abi.FP32_SPLIT16))
    out = []
    for L in (0, 1):
        with Engine(games=3, sims=200, c_puct=math.sqrt(2.0), train_noise=0, leaf_batch=L, **kw) as e:
            if evaluator == "nn":
                e.load_weights(trained3)
            r = e.search(roots)
            assert e.nn_fallbacks() == 0
            out.append((r.moves.tobytes(), r.pi.tobytes(), [e.tree(g).tobytes() for g in range(3)],
                        (r.stats.sims, r.stats.expansions, r.stats.children, r.stats.terminal_leaves, r.stats.depth_sum,
                         r.stats.stuck_leaves, r.stats.max_nodes, r.stats.nn_evals)))
            assert e.leaf_batch_stats() == ((200 * 3, 200 * 3, 0) if L else (0, 0, 0))
    assert out[0] == out[1]


def test_network_tree_equals_the_rule(orc, trained3):
    """The trained 3-block network, L = 8, 64 playouts: the rule's evaluator is one batch-1 forward of the GPU
    network per leaf (a tile's rows are independent), and no tile left the fp16 range."""
    roots = np.concatenate([start_root(orc, 0), midgame_roots(orc, 3)[1:2]])
    with Engine(games=2, sims=64, c_puct=math.sqrt(2.0), train_noise=0, evaluator=_abi.EVAL_NN, blocks=3,
                precision=_abi.FP32_SPLIT16, leaf_batch=8) as e, \
            Engine(games=4, sims=1, blocks=3, precision=_abi.FP32_SPLIT16) as ev:
        e.load_weights(trained3)
        ev.load_weights(trained3)

        def evaluator(gs):
            p, v = ev.nn_forward(lbr.state_np(gs, _abi.STATE_DTYPE))
            return [float(x) for x in p.reshape(-1)], float(v[0])

        r = _check_search(e, roots, 64, math.sqrt(2.0), 8, evaluator)
        assert e.nn_fallbacks() == 0 and ev.nn_fallbacks() == 0
        assert r.stats.sims == 128 and e.leaf_batch_stats()[0] < 128  # rounds of more than one leaf


@pytest.mark.parametrize("L", [1, 7])
def test_network_recompute_tree_equals_the_rule(orc, trained3, L):
    """Every evaluation leaves the fp16 range (the trained 3-block blob with the BN-folded first-layer bias at 1e5,
    as test_one_launch_search_equals_step_launches' nn_overflow rows), so every round's tile takes the in-kernel
    recompute: one-leaf rounds (L = 1) and an odd partial tile (L = 7), 3L + 5 playouts. The rule's evaluator is
    one batch-1 forward per leaf of a second engine with the same weights; every round is counted as one
    recomputed tile; and L = 1 is the leaf_batch = 0 search (k_search_lat's recompute) on the same weights."""
    from onitama_az.weights import blob_from_named, named_from_blob
    named = {k: v.copy() for k, v in named_from_blob(trained3.copy(), 3).items()}
    named["bn1|bias"][:] = 1.0e5  # first-layer activations ~1e5 > 65504
    bad = blob_from_named(named, 3)
    roots = np.concatenate([start_root(orc, 0), midgame_roots(orc, 3)[1:2]])
    sims, c = 3 * L + 5, math.sqrt(2.0)
    kw = dict(games=2, sims=sims, c_puct=c, train_noise=0, evaluator=_abi.EVAL_NN, blocks=3,
              precision=_abi.FP32_SPLIT16)

    def dump(e, r):
        return (r.moves.tobytes(), r.pi.tobytes(), [e.tree(g).tobytes() for g in range(2)],
                (r.stats.sims, r.stats.expansions, r.stats.children, r.stats.terminal_leaves, r.stats.depth_sum,
                 r.stats.stuck_leaves, r.stats.max_nodes, r.stats.nn_evals))

    with Engine(leaf_batch=L, **kw) as e, Engine(games=4, sims=1, blocks=3, precision=_abi.FP32_SPLIT16) as ev:
        e.load_weights(bad)
        ev.load_weights(bad)

        def evaluator(gs):
            p, v = ev.nn_forward(lbr.state_np(gs, _abi.STATE_DTYPE))
            return [float(x) for x in p.reshape(-1)], float(v[0])

        r = _check_search(e, roots, sims, c, L, evaluator)
        rounds = e.leaf_batch_stats()[0]
        assert rounds > 0 and e.nn_fallbacks() == rounds  # a round is never empty and every tile overflows
        par = dump(e, r)
    if L == 1:
        with Engine(leaf_batch=0, **kw) as e:
            e.load_weights(bad)
            assert dump(e, e.search(roots)) == par


def test_search_time_budget_stops_at_a_round(orc):
    """A budget far below one search (1 us): each root stops at a round boundary with 1 <= playouts <= sims, its
    root visits are the reported playouts and no in-flight count is left. An ample budget (10 s) gives exactly
    the unbudgeted tree."""
    roots, sims, L, c = midgame_roots(orc, 3), 400, 4, 5.0
    with Engine(games=3, sims=sims, c_puct=c, train_noise=0, evaluator=_abi.EVAL_HASH, blocks=0, leaf_batch=L) as e:
        e.set_search_time(1e-6)
        r = e.search(roots)
        n = e.search_playouts(3)
        assert np.all((n >= 1) & (n < sims)), n
        for g in range(3):
            t = e.tree(g)
            assert int(t["N"][0]) == int(n[g]) and not t["pad"].any()
        assert r.stats.sims == int(n.sum()) == e.leaf_batch_stats()[1] and e.last_sims() == int(n.max())
        e.set_search_time(10.0)
        _check_search(e, roots, sims, c, L)
        e.set_search_time(0.0)
        _check_search(e, roots, sims, c, L)


@pytest.mark.parametrize("bad", [dict(step_kernels=1), dict(compact=1), dict(compact=2), dict(reuse_visits=64),
                                 dict(evaluator=_abi.EVAL_NN, blocks=1, precision=_abi.FP32),
                                 dict(evaluator=_abi.EVAL_NN, blocks=1, precision=_abi.BF16),
                                 dict(evaluator=_abi.EVAL_NN, blocks=1, precision=_abi.FP32_SPLIT),
                                 dict(leaf_batch=17)],
                         ids=["step_kernels", "compact1", "compact2", "reuse_visits", "fp32", "bf16", "bf16x6", "L17"])
def test_creation_refuses_what_could_never_run(bad):
    kw = dict(games=2, sims=32, c_puct=5.0, train_noise=0, evaluator=_abi.EVAL_HASH, blocks=0, leaf_batch=4)
    kw.update(bad)
    with pytest.raises(_abi.OazError, match="leaf_batch"):
        Engine(**kw)
    kw.update(leaf_batch=0)  # the same configuration without the feature is an engine
    Engine(**kw).close()


def test_searches_it_cannot_take_fail_without_a_launch(orc, lib):
    """Root noise, more roots than CUs and self-play are OAZ_ERR_STATE with a message, nothing is launched, and the
    next valid search on the same engine still equals the rule."""
    import re
    roots, sims, L, c, cap = midgame_roots(orc, 3), 40, 7, 5.0, 1024  # (no device here has 1 024 CUs)
    many = np.concatenate([roots] * (cap // 3 + 1))[:cap]
    moves, pi = np.zeros(cap, dtype=_abi.MOVE_DTYPE), np.zeros((cap, 50), dtype=np.float32)

    def refused(rc, what):
        assert rc == _abi.ERR_STATE and what in lib.oaz_last_error() and b"leaf_batch" in lib.oaz_last_error()

    def search(G):
        return lib.oaz_search(e.handle, _abi.ptr(many), G, _abi.ptr(moves), _abi.ptr(pi), None, None)

    with Engine(games=cap, sims=sims, c_puct=c, train_noise=0, evaluator=_abi.EVAL_HASH, blocks=0, leaf_batch=L) as e:
        e.set_timing(1)
        refused(search(cap), b"roots")
        cus = int(re.search(rb"at most (\d+) roots", lib.oaz_last_error()).group(1))
        assert 1 <= cus < cap
        refused(search(cus + 1), b"roots")
        e.set_search_params(sims, c, True)
        refused(search(3), b"root noise")
        e.set_search_params(sims, c, False)
        refused(lib.oaz_selfplay_reset(e.handle), b"self-play")
        refused(lib.oaz_selfplay_step(e.handle, 1), b"self-play")
        refused(lib.oaz_selfplay_run(e.handle, 1, None, 0, None, None), b"self-play")
        k = e.kernel_times()
        assert (k.backup_select_n, k.select_n, k.nn_n, k.expand_n, k.noise_n, k.finalize_n) == (0, 0, 0, 0, 0, 0)
        assert e.leaf_batch_stats() == (0, 0, 0)
        _check_search(e, roots, sims, c, L)
        r = e.search(many[:cus])  # CU-count roots are taken: one workgroup each
        for g in range(cus):
            mv, rpi, nodes, _ = _ref(many[g], sims, c, L)
            assert np.array_equal(r.pi[g].reshape(-1), rpi) and _mv(r.moves[g]) == mv, g
            if g in (0, cus // 2, cus - 1):
                assert_tree_equals(e.tree(g), nodes)
        assert r.stats.sims == cus * sims and e.leaf_batch_stats()[1] == cus * sims
        assert e.kernel_times().backup_select_n == 2
