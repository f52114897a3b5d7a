"""GPU: self-play temperature (oaz_config.temperature_plies, oaz_search_sample_moves) against the unchanged oracle.
The device's draw is compared with the rule restated in tests/temperature_util.py at the wave widths where a scan
can go wrong, and whole self-play games (with and without tree reuse, root noise, two ranks) with games predicted
from orc.search alone. Every condition on the cases themselves (lanes covered, games that differ from T = 0, kept
subtrees of a drawn child) is checked on the oracle's prediction, whose trees equal the GPU's. HASH evaluator and
blocks = 0."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import oracle_ffi
import temperature_util as tu
from conftest import kat_state, random_positions
from onitama_az import _abi
from onitama_az.engine import Engine
from tree_reuse_util import assert_trees_equal, best_child, children, mv_tuple, sorted_rows, unpack, usable_roots

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu

HASH = dict(evaluator=_abi.EVAL_HASH, blocks=0)
DECK = [0, 1, 2, 3, 4]
SEED = 4242


def _wide_root(orc):
    """A seeded position with K >= 33 legal moves (two in 8 000 random positions have as many)."""
    r = random_positions(orc, 7, seed=3023)[6:7].copy()
    assert len(orc.movegen(r)) >= 33 and orc.current_state(r) not in (1, 2)
    return r


def _stuck_root():
    kats = json.loads((ROOT / "tests" / "golden" / "reference_kats.json").read_text())
    case = [c for c in kats["movegen"] if "no_legal_moves_at_all" in c["src"]][0]
    return kat_state(case["state"], 1)  # Blue has no legal move (state.rs:852-889)


def _expected(orc, tree, pos, seed, gid, ply):
    """(child, move) oaz_search_sample_moves returns for this tree: the draw, the last maximum where no child has a
    visit, the pass and -1 without a child."""
    k = best_child(tree)
    if k is None:
        return -1, (25, 25, 0, 2 if int(pos["to_move"][0]) else 0)
    d = tu.pick(orc, seed, gid, ply, children(tree)["N"])
    k = k if d is None else d
    return k, unpack(children(tree)[k]["mv"])


def _pairs(g):
    """64 (game id, ply) pairs per root: small and 64-bit ids, every ply a self-play game can have."""
    rng = np.random.RandomState(100 + g)
    gids = np.concatenate([np.arange(40, dtype=np.uint64) + np.uint64(1000 * g),
                           rng.randint(0, 2 ** 62, size=24).astype(np.uint64) + np.uint64(2 ** 32)])
    plies = np.concatenate([np.arange(40, dtype=np.uint32) % 8, rng.randint(0, 256, size=24).astype(np.uint32)])
    return gids, plies


def test_t4_device_draw_equals_host_draw(orc):
    sims, c_puct, seed = 200, 5.0, 20260107
    roots = np.concatenate([usable_roots(orc, 10, seed=2101), _wide_root(orc), _stuck_root()])
    G = len(roots)
    assert G == 12
    refs = [tu.search_tree(orc, roots[g:g + 1], sims, c_puct, seed)[1] for g in range(G)]
    assert len(children(refs[10])) >= 33 and len(children(refs[11])) == 0
    pairs = [_pairs(g) for g in range(G)]
    # (the oracle's alone) the expected picks lie in lanes 0-15, 16-31 and >= 32, and one root passes
    want = [[_expected(orc, refs[g], roots[g:g + 1], seed, int(pairs[g][0][i]), int(pairs[g][1][i])) for g in range(G)]
            for i in range(64)]
    lanes = {min(c, 32) // 16 if c >= 0 else None for row in want for c, _ in row}
    assert lanes == {0, 1, 2, None}, lanes
    with Engine(games=G, sims=sims, c_puct=c_puct, seed=seed, train_noise=0, **HASH) as e:
        e.search(roots)
        trees = [e.tree(g) for g in range(G)]
        for g in range(G):
            assert_trees_equal(trees[g], refs[g])
        for i in range(64):
            gids = np.array([pairs[g][0][i] for g in range(G)], dtype=np.uint64)
            plies = np.array([pairs[g][1][i] for g in range(G)], dtype=np.uint32)
            moves, child = e.sample_moves(gids, plies)
            for g in range(G):
                assert _expected(orc, trees[g], roots[g:g + 1], seed, int(gids[g]), int(plies[g])) == want[i][g]
                assert (int(child[g]), mv_tuple(moves[g])) == want[i][g], (g, i)
        assert trees[0].tobytes() == e.tree(0).tobytes()  # the call changes no tree
        # the call needs the last search's trees
        assert e._lib.oaz_search_sample_moves(e.handle, G + 1, _abi.ptr(np.zeros(G + 1, np.uint64)),
                                              _abi.ptr(np.zeros(G + 1, np.uint32)),
                                              _abi.ptr(np.zeros(G + 1, _abi.MOVE_DTYPE)), None) == _abi.ERR_STATE
        assert e._lib.oaz_search_sample_moves(e.handle, 1, None, None, None, None) == _abi.ERR_ARG
    # one playout: the root is expanded and no child has a visit (S = 0): the last maximum, child K - 1
    with Engine(games=2, sims=1, c_puct=c_puct, seed=seed, train_noise=0, **HASH) as e:
        e.search(roots[9:11])
        for g in range(2):
            tree = e.tree(g)
            K = len(children(tree))
            assert K > 0 and int(children(tree)["N"].sum()) == 0
        moves, child = e.sample_moves(np.array([5, 6], np.uint64), np.array([0, 3], np.uint32))
        for g in range(2):
            kids = children(e.tree(g))
            assert int(child[g]) == len(kids) - 1 and mv_tuple(moves[g]) == unpack(kids[-1]["mv"])


@functools.lru_cache(maxsize=None)
def _predicted(fixed, max_plies, sims, R, T, train_noise, n_games=24, seed=SEED):
    """The n_games games from orc.search alone: (records, move sequences, summed info)."""
    recs, seqs, info = [], [], {}
    for gid in range(n_games):
        s, mv, i = tu.predicted_selfplay_game(oracle_ffi, gid, sims, 5.0, R, max_plies, seed, T,
                                              deck=np.array(DECK, np.uint8) if fixed else None, train_noise=train_noise)
        recs.append(s)
        seqs.append(mv)
        info = {k: info.get(k, 0) + v for k, v in i.items()}
    return np.concatenate(recs), tuple(seqs), info


def _selfplay(fixed, max_plies, sims, R, T, train_noise, slots=8, n_games=24, rank=0, world=1, seed=SEED):
    with Engine(games=slots, sims=sims, c_puct=5.0, max_plies=max_plies, seed=seed, fixed_deck=int(fixed), deck=DECK,
                reuse_visits=R, temperature_plies=T, train_noise=train_noise, rank=rank, world=world, **HASH) as e:
        got, st = e.selfplay_run(n_games, cap=n_games * (max_plies + 2))
        return got, st, e.temperature_stats(), e.reuse_stats()


def _check_against_prediction(fixed, max_plies, sims, R, T, train_noise):
    ref, seqs, info = _predicted(fixed, max_plies, sims, R, T, train_noise)
    _, seqs0, _ = _predicted(fixed, max_plies, sims, R, 0, train_noise)
    # (the oracle's alone) at least half of the games differ from the games without temperature
    assert sum(a != b for a, b in zip(seqs, seqs0)) >= 12
    got, st, ts, rs = _selfplay(fixed, max_plies, sims, R, T, train_noise)
    assert st.games_finished == 24
    assert len(got) == len(ref)
    assert np.array_equal(sorted_rows(got), sorted_rows(ref))
    assert ts == (info["draws"], info["differ"]) and ts[0] > 0 and ts[1] > 0
    return info, rs


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("max_plies", [10, 150])
@pytest.mark.parametrize("T", [4, 255])
def test_t5_selfplay_equals_the_oracle_loop(orc, T, max_plies, fixed):
    """24 games on 8 slots, records (z included) as sorted byte rows and the two counters."""
    _check_against_prediction(fixed, max_plies, 32, 0, T, 0)


def test_t5_selfplay_with_root_noise(orc):
    _check_against_prediction(True, 150, 32, 0, 4, 1)


@pytest.mark.parametrize("T", [4, 255])
def test_t6_tree_reuse_keeps_the_sampled_childs_subtree(orc, T):
    info, rs = _check_against_prediction(True, 150, 32, 96, T, 0)
    assert (rs.trees_kept, rs.trees_fresh) == (info["kept"], info["fresh"])
    assert info["kept_other"] >= 1  # a kept subtree of a child that is not the arg-max


def test_t7_rank_independence(orc):
    """Two ranks of 12 games each hold together the records of one engine playing the 24."""
    args = (True, 150, 32, 0, 4, 0)
    whole = _selfplay(*args)[0]
    parts = [_selfplay(*args, slots=4, rank=r, world=2) for r in range(2)]
    assert [p[1].games_finished for p in parts] == [12, 12]
    both = np.concatenate([p[0] for p in parts])
    assert np.array_equal(sorted_rows(both), sorted_rows(whole))
    assert np.array_equal(sorted_rows(whole), sorted_rows(_predicted(*args)[0]))
    info = _predicted(*args)[2]
    assert tuple(sum(p[2][k] for p in parts) for k in range(2)) == (info["draws"], info["differ"])
