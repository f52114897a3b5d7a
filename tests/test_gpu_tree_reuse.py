"""GPU: tree reuse (oaz_config.reuse_visits, oaz_search_advance / oaz_search_resume, self-play that keeps the
played move's subtree) against the unchanged oracle. The invariant (DESIGN.md "Tree reuse"): a root child's
subtree equals the oracle's fresh search of N_c playouts from the child's position, so a search resumed on it
for `sims` playouts equals a fresh search of N_c + sims, and a whole self-play game with reuse is predicted by
orc.search alone (tests/tree_reuse_util.py). HASH evaluator, no root noise and blocks = 0 unless stated."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import kat_state
from onitama_az import _abi
from onitama_az.engine import Engine
from tree_reuse_util import (assert_trees_equal, best_child, children, fresh_search, kept_visits,
                             least_visited_child, mv_tuple, predicted_selfplay_game, sorted_rows, stepped, unpack,
                             usable_roots)

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu

HASH = dict(train_noise=0, evaluator=_abi.EVAL_HASH, blocks=0)
FRESH = np.zeros(1, dtype=_abi.NODE_DTYPE)  # what k_tree_reset writes: a root with P = 1
FRESH["P"] = 1.0


def _rebase_host(lib, nodes, child):
    out = np.zeros(len(nodes), dtype=_abi.NODE_DTYPE)
    n = C.c_int(0)
    assert lib.oaz_tree_rebase_host(_abi.ptr(np.ascontiguousarray(nodes)), len(nodes), child, _abi.ptr(out), len(out),
                                    C.byref(n)) == 0
    return out[:n.value]


def _advance_and_check(e, orc, lib, trees, pos, picks, sims, c_puct, R):
    """advance() at the root's picks[g]-th child (None: the pass of a root without a child) of every game, checked
    against the keep rule, the host restatement and the oracle. Returns (kept, the stepped positions)."""
    G = len(pos)
    moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
    want_kept, nxt = np.zeros(G, dtype=np.int32), []
    for g in range(G):
        if picks[g] is None:
            mv = (25, 25, 0, 2 if int(pos[g]["to_move"]) else 0)
        else:
            mv = unpack(children(trees[g])[picks[g]]["mv"])
            want_kept[g] = kept_visits(orc, trees[g], pos[g:g + 1], picks[g], sims, R)
        moves[g] = mv
        nxt.append(stepped(orc, pos[g:g + 1], mv)[0])
    nxt = np.concatenate(nxt)
    kept = e.advance(moves)
    assert np.array_equal(kept, want_kept), (kept, want_kept)
    for g in range(G):
        t = e.tree(g)
        if kept[g] == 0:
            assert t.tobytes() == FRESH.tobytes(), g
            continue
        assert kept[g] == children(trees[g])[picks[g]]["N"]
        assert t.tobytes() == _rebase_host(lib, trees[g], picks[g]).tobytes(), g
        assert_trees_equal(t, fresh_search(orc, nxt[g:g + 1], int(kept[g]), c_puct)[2])
    return kept, nxt


def _check_search(e, orc, r, pos, playouts, c_puct, tree_games=None):
    """The engine's trees, pi and moves equal the oracle's fresh searches of playouts[g] from pos[g]. Where a
    chained game's root is already won (the move before won: the game is over, the chain goes on regardless),
    node 0's W is outside the invariant: the root's parent colour enters the terminal reward, and a kept root
    had a parent where a fresh one has none. Every other field and node is compared there too."""
    trees = []
    for g in range(len(pos)):
        mv, pi, ref = fresh_search(orc, pos[g:g + 1], int(playouts[g]), c_puct)
        assert np.array_equal(r.pi[g], pi), g
        assert mv_tuple(r.moves[g]) == mv_tuple(mv), g
        if tree_games is None or g in tree_games:
            got = e.tree(g)
            if orc.current_state(pos[g:g + 1]) in (1, 2) and len(got):
                got["W"][0] = ref["W"][0]
            assert_trees_equal(got, ref)
        trees.append(ref)
    return trees


@pytest.mark.parametrize("pick", ["best", "least"])
def test_g1_advance_rebases_the_trees(lib, orc, pick):
    G, sims, c_puct, R = 12, 64, 2.0, 192
    roots = usable_roots(orc, G, seed=2101)
    with Engine(games=G, sims=sims, c_puct=c_puct, reuse_visits=R, **HASH) as e:
        r = e.search(roots)
        trees = [e.tree(g) for g in range(G)]
        for g in range(G):
            assert_trees_equal(trees[g], fresh_search(orc, roots[g:g + 1], sims, c_puct)[2])
        picks = [best_child(t) if pick == "best" else least_visited_child(t) for t in trees]
        if pick == "best":
            assert [mv_tuple(m) for m in r.moves] == [unpack(children(t)[k]["mv"]) for t, k in zip(trees, picks)]
        kept, nxt = _advance_and_check(e, orc, lib, trees, roots, picks, sims, c_puct, R)
        assert (kept > 0).sum() >= G // 2
        res = e.resume(G)
        assert res.roots.tobytes() == nxt.tobytes()
        st = e.reuse_stats()
        assert (st.trees_kept, st.trees_fresh, st.visits_kept) == ((kept > 0).sum(), (kept == 0).sum(), kept.sum())


@pytest.mark.parametrize("games,step_kernels,compact,parts,sims,R", [
    (1, 0, 0, 0, 64, 80), (12, 0, 0, 0, 64, 80), (12, 1, 0, 0, 64, 80), (300, 0, 0, 0, 64, 80), (26, 0, 1, 2, 64, 80),
    (6, 0, 0, 0, 400, 1200)])  # the last: trees of thousands of nodes (about a hundred 64-node chunks to re-root)
def test_g2_resume_equals_a_fresh_search_of_kept_plus_sims(lib, orc, games, step_kernels, compact, parts, sims, R):
    """search, then twice advance + resume, at the sizes of the three search paths (one workgroup per game, 16
    games per workgroup, per-step launches) and with leaf compaction on two game parts. reuse_visits = sims + 16:
    a child is kept when N_c <= 16, which the most visited children of these searches (about 5 to 50 visits)
    meet in some games and miss in others, so the chain takes both branches of the keep rule at every size
    (the one-game case keeps at its first advance and starts afresh, for capacity, at its second)."""
    c_puct = 2.0
    roots = usable_roots(orc, games, seed=2200 + games)
    some = None if games <= 26 else set(range(0, games, 23)) | {games - 1}  # trees compared (pi and moves: all)
    with Engine(games=games, sims=sims, c_puct=c_puct, reuse_visits=R, step_kernels=step_kernels, compact=compact,
                parts=parts, **HASH) as e:
        r = e.search(roots)
        pos, playouts = roots, np.full(games, sims)
        took = {"kept": 0, "fresh": 0, "fresh for capacity": 0}
        for stage in range(2):
            trees = _check_search(e, orc, r, pos, playouts, c_puct, some)
            want, nxt = np.zeros(games, dtype=np.int32), []
            for g in range(games):
                k = best_child(trees[g])
                assert mv_tuple(r.moves[g]) == ((25, 25, 0, 2 if int(pos[g]["to_move"]) else 0) if k is None
                                                else unpack(children(trees[g])[k]["mv"]))
                want[g] = 0 if k is None else kept_visits(orc, trees[g], pos[g:g + 1], k, sims, R)
                nxt.append(stepped(orc, pos[g:g + 1], mv_tuple(r.moves[g]))[0])
            kept = e.advance(r.moves)
            assert np.array_equal(kept, want)
            took["kept"] += int((kept > 0).sum())
            took["fresh"] += int((kept == 0).sum())
            took["fresh for capacity"] += sum(1 for g in range(games) if kept[g] == 0 and best_child(trees[g]) is not None and
                                              kept_visits(orc, trees[g], pos[g:g + 1], best_child(trees[g]), sims, 10 ** 6))
            pos, playouts = np.concatenate(nxt), kept + sims
            r = e.resume(games)
            assert r.roots.tobytes() == pos.tobytes()
            assert r.stats.sims == games * sims and e.last_sims() == sims
        _check_search(e, orc, r, pos, playouts, c_puct, some)
        assert took["kept"] > 0 and (R != 80 or min(took.values()) > 0), took


def _selfplay_with_reuse(orc, fixed, max_plies, sims, R, slots=8, n_games=24, seed=4242):
    deck = [0, 1, 2, 3, 4]
    with Engine(games=slots, sims=sims, c_puct=5.0, max_plies=max_plies, seed=seed, fixed_deck=int(fixed), deck=deck,
                reuse_visits=R, **HASH) as e:
        got, st = e.selfplay_run(n_games, cap=n_games * (max_plies + 2))
        rs = e.reuse_stats()
    assert st.games_finished == n_games
    ref, n_kept, n_fresh = [], 0, 0
    for gid in range(n_games):
        s, a, b = predicted_selfplay_game(orc, gid, sims, 5.0, R, max_plies, seed,
                                          deck=np.array(deck, np.uint8) if fixed else None)
        ref.append(s)
        n_kept, n_fresh = n_kept + a, n_fresh + b
    ref = np.concatenate(ref)
    assert len(got) == len(ref)
    assert np.array_equal(sorted_rows(got), sorted_rows(ref))
    return rs, n_kept, n_fresh


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("max_plies", [10, 150])
def test_g3_selfplay_equals_the_oracle_loop(orc, fixed, max_plies):
    """24 games on 8 slots (every slot goes on into its second and third game, which start on fresh trees)."""
    rs, n_kept, n_fresh = _selfplay_with_reuse(orc, fixed, max_plies, sims=32, R=96)
    assert rs.trees_kept > 0 and rs.trees_fresh > 0
    # the quota's last plies aside (slots that have finished their games count nothing), the counters are the loop's
    assert (rs.trees_kept, rs.trees_fresh) == (n_kept, n_fresh)


def test_g3_selfplay_with_almost_no_room_to_keep(orc):
    rs, n_kept, n_fresh = _selfplay_with_reuse(orc, True, 150, sims=32, R=33)  # kept only when N_c <= 1
    assert (rs.trees_kept, rs.trees_fresh) == (n_kept, n_fresh) and n_fresh > 20 * max(n_kept, 1)


def _rc_advance(e, moves, G=None):
    moves = np.ascontiguousarray(moves, dtype=_abi.MOVE_DTYPE)
    return e._lib.oaz_search_advance(e.handle, _abi.ptr(moves), len(moves) if G is None else G, None)


def test_g4_guards(lib, orc):
    G, sims = 6, 32
    roots = usable_roots(orc, G, seed=2404)
    with Engine(games=G, sims=sims, c_puct=2.0, **HASH) as e:  # reuse_visits = 0
        r = e.search(roots)
        assert _rc_advance(e, r.moves) == _abi.ERR_STATE
        assert e._lib.oaz_search_resume(e.handle, G, None, None, None, None, None) == _abi.ERR_STATE
        st = e.reuse_stats()
        assert (st.trees_kept, st.trees_fresh, st.visits_kept, st.nodes_kept) == (0, 0, 0, 0)
    with Engine(games=G, sims=sims, c_puct=2.0, reuse_visits=96, **HASH) as e:
        assert _rc_advance(e, np.zeros(1, dtype=_abi.MOVE_DTYPE)) == _abi.ERR_STATE  # no search yet
        r = e.search(roots[:4])
        assert _rc_advance(e, np.zeros(5, dtype=_abi.MOVE_DTYPE)) == _abi.ERR_STATE  # G larger than the last search
        # a move that is no root child: OAZ_ERR_ARG, the trees and the resident roots stay byte-identical
        before = [e.tree(g).tobytes() for g in range(4)]
        bad = r.moves.copy()
        legal = {mv_tuple(m) for m in orc.movegen(roots[2:3])}
        bad[2] = next((f, t, p, s) for f in range(25) for t in range(25) for p in (0, 1) for s in range(4)
                      if (f, t, p, s) not in legal)
        assert _rc_advance(e, bad) == _abi.ERR_ARG and b"move 2" in lib.oaz_last_error()
        bad[2] = (25, 25, 0, 2 if int(roots[2]["to_move"]) else 0)  # a pass at a root that has children
        assert _rc_advance(e, bad) == _abi.ERR_ARG
        assert [e.tree(g).tobytes() for g in range(4)] == before
        kept = e.advance(r.moves)  # (the resident roots are still the searched ones: the advance steps from them)
        res = e.resume(4)
        want = np.concatenate([stepped(orc, roots[g:g + 1], mv_tuple(r.moves[g]))[0] for g in range(4)])
        assert res.roots.tobytes() == want.tobytes()
        # a second resume without an advance would pass reuse_visits root visits: kept + 32 + 32 + 32 > 96
        assert kept.max() > 0
        assert e._lib.oaz_search_resume(e.handle, 4, None, None, None, None, None) == 0
        assert e._lib.oaz_search_resume(e.handle, 4, None, None, None, None, None) == _abi.ERR_STATE
        e.selfplay_step(1)
        assert _rc_advance(e, res.moves) == _abi.ERR_STATE  # self-play ran in between
        assert e._lib.oaz_search_resume(e.handle, 4, None, None, None, None, None) == _abi.ERR_STATE


def test_g4_pass_and_winning_move_leave_fresh_trees(lib, orc):
    kats = json.loads((ROOT / "tests" / "golden" / "reference_kats.json").read_text())
    case = [c for c in kats["movegen"] if "no_legal_moves_at_all" in c["src"]][0]
    stuck = kat_state(case["state"], 1)  # Blue has no legal move (state.rs:852-889)
    tactic = kats["tactics"][0]          # a win in one (mcts_arena.rs:459-483)
    won_by = kat_state(tactic["state"], tactic["color"])
    roots = np.concatenate([stuck, won_by])
    with Engine(games=2, sims=20, c_puct=5.0, reuse_visits=60, **HASH) as e:
        r = e.search(roots)
        assert mv_tuple(r.moves[0]) == (25, 25, 0, 2)
        moves = r.moves.copy()
        moves[1] = tuple(tactic["expected"])
        assert stepped(orc, won_by, tuple(tactic["expected"]))[1] in (1, 2)
        wrong = moves.copy()
        wrong[0] = (25, 25, 0, 0)  # a pass with a card of the side that is not to move
        assert _rc_advance(e, wrong) == _abi.ERR_ARG
        kept = e.advance(moves)
        assert list(kept) == [0, 0]
        assert e.tree(0).tobytes() == FRESH.tobytes() and e.tree(1).tobytes() == FRESH.tobytes()
        res = e.resume(2)
        want = np.concatenate([stepped(orc, roots[g:g + 1], mv_tuple(moves[g]))[0] for g in range(2)])
        assert res.roots.tobytes() == want.tobytes()
        assert list(want[0]["cards"]) == [case["state"]["deck"][i] for i in (0, 1, 4, 3, 2)] and want[0]["to_move"] == 0
        assert_trees_equal(e.tree(0), fresh_search(orc, want[0:1], 20, 5.0)[2])
        st = e.reuse_stats()
        assert (st.trees_kept, st.trees_fresh) == (0, 2)


def test_g5_noise_is_reproducible_and_a_budgeted_ply_completes():
    kw = dict(games=8, sims=24, c_puct=5.0, train_noise=1, evaluator=_abi.EVAL_HASH, blocks=0, max_plies=20, seed=77,
              reuse_visits=72)
    runs = []
    for _ in range(2):
        with Engine(**kw) as e:
            got, st = e.selfplay_run(8, cap=8 * 22)
            rs = e.reuse_stats()
            runs.append((got.tobytes(), rs.trees_kept, rs.visits_kept))
    assert runs[0] == runs[1] and runs[0][1] > 0 and len(runs[0][0]) > 0
    with Engine(**dict(kw, search_time_ns=10 ** 9)) as e:
        e.selfplay_step(2)  # the second ply begins on kept trees
        e.sync()
        assert 1 <= e.last_sims() <= 24
        assert e.selfplay_stats().moves == 16 and e.reuse_stats().trees_kept > 0


def test_g6_off_means_off(orc):
    """reuse_visits = 0 is the engine without the feature: the same samples as a config whose last word was
    never named (zero-initialised, as a caller built against the header before the field had a name), which
    are the oracle's games; nothing is counted and no tree is ever kept."""
    kw = dict(games=8, sims=12, c_puct=5.0, max_plies=150, seed=4242, fixed_deck=0, **HASH)
    with Engine(reuse_visits=0, **kw) as e:
        a, st = e.selfplay_run(16, cap=16 * 152)
        rs = e.reuse_stats()
    cfg = _abi.default_config()
    assert bytes(cfg)[116:120] == b"\0\0\0\0"
    with Engine(config=cfg, **kw) as e:
        b, _ = e.selfplay_run(16, cap=16 * 152)
    assert a.tobytes() == b.tobytes() and st.games_finished == 16
    assert (rs.trees_kept, rs.trees_fresh, rs.visits_kept, rs.nodes_kept) == (0, 0, 0, 0)
    ref = np.concatenate([orc.selfplay_game(orc.search_cfg(sims=12, c_puct=5.0, evaluator=orc.EVAL_HASH, seed=4242), gid,
                                            max_plies=150)[0] for gid in range(16)])
    assert np.array_equal(sorted_rows(a), sorted_rows(ref))
