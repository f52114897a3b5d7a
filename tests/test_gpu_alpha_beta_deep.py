"""GPU: the split alpha-beta search (oaz_alphabeta_generate_move: expand, search, fold in csrc/oaz_alphabeta.hip)
against the CPU restatement's goldens (tests/golden/alphabeta_kats.json, alphabeta_deep_kats.json), its clock,
and the tournament over it. Moves and scores are integers and compare exactly. Each search runs once."""
import numpy as np
import pytest

import alphabeta_deep_golden as D
import alphabeta_golden as G
from onitama_az import _abi
from onitama_az import alpha_beta as ab_mod
from onitama_az.alpha_beta import AlphaBeta, alpha_beta_generate_move, alpha_beta_search
from onitama_az.arena import NativeRandomAgent
from onitama_az.evaluator import AlphaZeroAgent, EvaluatorConfig, fight
from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNet, ConvResNetConfig
from onitama_az.pure_mcts import Mcts
from onitama_az.tournament import AGENTS, PAIRINGS, Tournament, fold_pairing

pytestmark = pytest.mark.gpu


def _mismatch(res, want_mv, want_sc):
    bad = [i for i in range(len(want_mv)) if res.moves[i].tobytes() != want_mv[i].tobytes() or res.scores[i] != want_sc[i]]
    return [(i, res.moves[i].tolist(), int(res.scores[i]), want_mv[i].tolist(), int(want_sc[i])) for i in bad[:6]]


def _same(a, b):
    return a.moves.tobytes() == b.moves.tobytes() and np.array_equal(a.scores, b.scores)


@pytest.fixture(scope="module")
def depth4_split2():
    return alpha_beta_generate_move(G.load()["depth4"]["roots"], max_depth=4, split=2)


# ---- untimed, against the existing goldens ---------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 2, 3])
def test_depth4_goldens_at_every_split(split, depth4_split2):
    sec = G.load()["depth4"]
    r = depth4_split2 if split == 2 else alpha_beta_generate_move(sec["roots"], max_depth=4, split=split)
    assert len(r.moves) == 256 and not _mismatch(r, sec["move_np"], sec["score_np"])
    st = r.stats
    assert (st.iterations, st.plies, st.split) == (1, 3, min(split, 2))  # 3 plies: split 3 is clamped to 2
    assert st.items > 256 and st.positions > st.items and 0 < st.max_positions_per_root <= st.positions
    assert st.roots_without_move == 0 and st.elapsed_ms > 0


@pytest.mark.parametrize("split", [2, 3])
def test_depth6_goldens_at_split_2_and_3(split):
    sec = G.load()["depth6"]
    r = alpha_beta_generate_move(sec["roots"], max_depth=6, split=split)
    assert not _mismatch(r, sec["move_np"], sec["score_np"])
    assert (r.stats.plies, r.stats.split) == (5, split)


def test_auto_split_answers_as_the_explicit_ones_and_names_its_choice(depth4_split2):
    """256 roots x 12^2 fill the GPU at S = 2 (and 3 plies allow no more); 32 roots need S = 3."""
    r4 = alpha_beta_generate_move(G.load()["depth4"]["roots"], max_depth=4)
    assert _same(r4, depth4_split2) and r4.stats.split == 2 and r4.stats.items == depth4_split2.stats.items
    sec = G.load()["depth6"]
    r6 = alpha_beta_generate_move(sec["roots"], max_depth=6, split=0)
    assert not _mismatch(r6, sec["move_np"], sec["score_np"]) and r6.stats.split == 3


def test_the_old_entry_point_is_what_it_was(monkeypatch):
    """oaz_alphabeta_search answers max_depth 6 as before, the default AlphaBeta still goes through it, and
    k_alphabeta is still the library's kernel for it."""
    sec = G.load()["depth6"]
    r = alpha_beta_search(sec["roots"], max_depth=6)
    assert not _mismatch(r, sec["move_np"], sec["score_np"])
    deep = alpha_beta_generate_move(sec["roots"][:8], max_depth=6, split=1)
    old = alpha_beta_search(sec["roots"][:8], max_depth=6)
    assert deep.stats.positions == old.stats.positions  # split 1 is k_alphabeta's split: the same positions
    monkeypatch.setattr(ab_mod, "alpha_beta_generate_move", lambda *a, **k: pytest.fail("the default path changed"))
    assert AlphaBeta().generate_moves_np(sec["roots"][:4]).tobytes() == sec["move_np"][:4].tobytes()
    assert AlphaBeta(max_depth=4, search_time=0.4).generate_moves_np(G.load()["depth4"]["roots"][:4]).tobytes() == \
        G.load()["depth4"]["move_np"][:4].tobytes()
    assert b"k_alphabeta" in _abi.LIB_PATH.read_bytes()


# ---- the hand-built positions: nodes without a move and winning moves at every level -------------------------------
@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("max_depth", [3, 4, 5, 6, 7, 8])
def test_hand_built_positions_at_every_depth_and_split(max_depth, split):
    d = D.load()
    k = max_depth - 3
    r = alpha_beta_generate_move(d["hand_roots"], max_depth=max_depth, split=split)
    for i, h in enumerate(d["hand"]):
        assert list(r.moves[i].tolist()) == h["move"][k] and int(r.scores[i]) == h["score"][k], (
            h["name"], r.moves[i], r.scores[i])
    assert r.stats.roots_without_move == 2 and r.stats.split == max(1, min(split, max_depth - 2))
    by = {h["name"]: i for i, h in enumerate(d["hand"])}
    assert r.moves[by["no_move_red"]].tolist() == (25, 25, 0, 0) and r.scores[by["no_move_red"]] == G.INT32_MIN
    assert r.moves[by["no_move_blue"]].tolist() == (25, 25, 0, 2) and r.scores[by["no_move_blue"]] == G.INT32_MAX
    assert r.scores[by["interior_no_move_blue_root"]] == G.INT32_MIN  # the sentinel travels up through the fold
    assert r.scores[by["interior_no_move_red_root"]] == G.INT32_MAX


@pytest.mark.parametrize("max_depth", [2, 3])
def test_split_3_is_clamped_at_one_and_two_plies(max_depth):
    d = D.load()
    roots = np.concatenate([d["hand_roots"], G.load()["depth4"]["roots"][:24]])
    r = alpha_beta_generate_move(roots, max_depth=max_depth, split=3)
    assert (r.stats.split, r.stats.plies) == (1, max_depth - 1)
    assert _same(r, alpha_beta_search(roots, max_depth=max_depth))
    if max_depth == 3:
        assert [m.tolist() for m in r.moves[:8]] == [tuple(h["move"][0]) for h in d["hand"]]


# ---- the depths only this entry point answers ------------------------------------------------------------------
def test_depth7_goldens_auto_split():
    sec = D.load()["depth7"]
    r = alpha_beta_generate_move(sec["roots"], max_depth=7)
    assert not _mismatch(r, sec["move_np"], sec["score_np"])
    assert (r.stats.iterations, r.stats.plies, r.stats.split) == (1, 6, 3)
    assert r.stats.positions > sum(sec["positions"])  # full windows visit more than the sequential search


def test_depth8_goldens_auto_split():
    sec = D.load()["depth8"]
    r = alpha_beta_generate_move(sec["roots"], max_depth=8)
    assert not _mismatch(r, sec["move_np"], sec["score_np"])
    assert (r.stats.plies, r.stats.split) == (7, 3) and r.stats.items > 4 * 100


def test_agent_class_routes_deep_searches_to_the_split_search():
    sec = D.load()["depth7"]
    assert AlphaBeta(max_depth=7).generate_moves_np(sec["roots"][3:5]).tobytes() == sec["move_np"][3:5].tobytes()
    assert AlphaBeta(max_depth=7, split=2).generate_moves_np(sec["roots"][7:8]).tobytes() == sec["move_np"][7:8].tobytes()


# ---- batch edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 65])
def test_batch_sizes_from_an_offset(n):
    sec = G.load()["depth4"]
    lo = 37
    r = alpha_beta_generate_move(sec["roots"][lo:lo + n], max_depth=4, split=2)
    assert len(r.moves) == n and not _mismatch(r, sec["move_np"][lo:lo + n], sec["score_np"][lo:lo + n])


@pytest.mark.parametrize("split", [1, 2])
def test_a_root_without_items_among_others(split):
    """A root without a legal move (no item at all), a mate in one (leaves inside the expansion) and ordinary
    roots in one call: the levels' offsets of the neighbours must not move."""
    hand = {h["name"]: h for h in G.load()["hand"]}
    sec = G.load()["depth4"]
    names = ["no_move_red", "mate_capture_red", "no_move_blue", "mate_temple_blue"]
    roots = np.concatenate([sec["roots"][0:2], G.states([hand[names[0]]["state"]]), sec["roots"][2:3],
                            G.states([hand[n]["state"] for n in names[1:3]]), sec["roots"][3:5],
                            G.states([hand[names[3]]["state"]])])
    want_mv = [sec["move"][0], sec["move"][1], hand[names[0]]["move"], sec["move"][2], hand[names[1]]["move"],
               hand[names[2]]["move"], sec["move"][3], sec["move"][4], hand[names[3]]["move"]]
    want_sc = [sec["score"][0], sec["score"][1], hand[names[0]]["score"], sec["score"][2], hand[names[1]]["score"],
               hand[names[2]]["score"], sec["score"][3], sec["score"][4], hand[names[3]]["score"]]
    r = alpha_beta_generate_move(roots, max_depth=4, split=split)
    assert [list(m.tolist()) for m in r.moves] == want_mv and r.scores.tolist() == want_sc
    assert r.stats.roots_without_move == 2


def test_one_root_per_call_equals_batched(depth4_split2):
    roots = G.load()["depth4"]["roots"]
    for i in range(0, 48):
        r = alpha_beta_generate_move(roots[i:i + 1], max_depth=4)
        assert r.moves[0].tobytes() == depth4_split2.moves[i].tobytes() and r.scores[0] == depth4_split2.scores[i], i
        assert r.stats.positions == r.stats.max_positions_per_root > 0 and r.stats.split == 2


# ---- the clock (mod.rs:145-156) --------------------------------------------------------------------------------
def test_clock_of_one_nanosecond_runs_the_first_iteration_only():
    roots = G.load()["depth6"]["roots"][:8]
    r = alpha_beta_generate_move(roots, max_depth=6, search_time=1e-9)
    assert (r.stats.iterations, r.stats.plies) == (1, 1)
    assert _same(r, alpha_beta_search(roots, max_depth=2))


def test_clock_that_does_not_run_out_reaches_max_depth():
    sec = G.load()["depth4"]
    roots = sec["roots"][:16]
    r = alpha_beta_generate_move(roots, max_depth=5, search_time=60.0)
    assert (r.stats.iterations, r.stats.plies) == (4, 4)
    assert _same(r, alpha_beta_search(roots, max_depth=5))
    assert _same(r, alpha_beta_generate_move(roots, max_depth=5))


def test_clock_of_5_ms_at_max_depth_8_ends_on_a_whole_iteration():
    roots = D.load()["depth8"]["roots"]
    r = alpha_beta_generate_move(roots, max_depth=8, search_time=0.005)
    assert 1 <= r.stats.plies <= 7 and r.stats.iterations == r.stats.plies
    assert _same(r, alpha_beta_generate_move(roots, max_depth=r.stats.plies + 1))


# ---- games ---------------------------------------------------------------------------------------------------
def test_alphabeta7_vs_random_games_equal_golden():
    g = D.load()["games"]
    st = fight(EvaluatorConfig(game_amnt=len(g["result"]), deck=None, max_plies=g["max_plies"], seed=g["seed"]),
               AlphaBeta(g["max_depth"]), NativeRandomAgent(g["seed"]))
    assert st.results == g["result"] and st.plies == g["plies"]


def test_four_agent_tournament():
    g = D.load()["games"]
    model = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=21)
    az = AlphaZeroAgent(AlphaZeroMctsConfig(search_time=1.0, exploration_c=1.0, max_playouts=16, train=False,
                                            enforce_search_time=False), model)
    t = Tournament(AlphaBeta(max_depth=g["max_depth"], enforce_search_time=False),
                   Mcts(search_time=1.0, min_node_visits=0, exploration_c=1.0, max_playouts=50, seed=g["seed"]), az,
                   NativeRandomAgent(g["seed"]), game_amnt=2, max_plies=g["max_plies"], seed=g["seed"], verbose=False)
    try:
        out = t.pit()
    finally:
        eng = model.__dict__.get("_search", {}).get("engine")
        if eng is not None:
            eng.close()
    assert [(p.agent, p.opponent) for p in out] == [(AGENTS[i], AGENTS[j]) for i, j in PAIRINGS]
    assert all(p.decks == t.decks and len(p.results) == len(p.plies) == 2 for p in out)
    assert all(1 <= n <= g["max_plies"] + 2 for p in out for n in p.plies)
    r = {k: 800.0 for k in AGENTS}
    for p in out:  # the ratings are chained through the fold, pairing after pairing
        r[p.agent], r[p.opponent], wins, cut = fold_pairing(p.results, r[p.agent], r[p.opponent])
        assert p.ratings == r and (p.wins, p.cut) == (wins, cut) and p.winrate == wins / 2
    assert t.ratings == r
    assert out[2].results == g["result"] and out[2].plies == g["plies"]  # AlphaBeta - Random: the golden games
