"""GPU: the batched alpha-beta search (csrc/oaz_alphabeta.hip through oaz_alphabeta_search) against the
CPU restatement's goldens (tests/golden/alphabeta_kats.json): moves and scores are integer arithmetic and
compare exactly. Each search runs once."""
import pytest

import alphabeta_golden as G
from onitama_az.alpha_beta import AlphaBeta, alpha_beta_search
from onitama_az.evaluator import Evaluator, EvaluatorConfig, fight
from onitama_az.game import ORIGINAL_CARDS, Deck, GameState
from onitama_az.mcts import ConvResNet, ConvResNetConfig

pytestmark = pytest.mark.gpu


def _mismatch(res, sec, lo=0, hi=None):
    """Indices where move or score differ from the golden slice [lo, hi)."""
    want_mv, want_sc = sec["move_np"][lo:hi], sec["score_np"][lo:hi]
    bad = [i for i in range(len(want_mv)) if res.moves[i].tobytes() != want_mv[i].tobytes() or res.scores[i] != want_sc[i]]
    return [(lo + i, res.moves[i].tolist(), int(res.scores[i]), want_mv[i].tolist(), int(want_sc[i])) for i in bad[:6]]


@pytest.fixture(scope="module")
def depth4_batched():
    return alpha_beta_search(G.load()["depth4"]["roots"], max_depth=4)


def test_depth3_batch_equals_golden(depth4_batched):
    sec = G.load()["depth4"]
    assert len(depth4_batched.moves) == 256
    assert not _mismatch(depth4_batched, sec)


def test_depth3_one_root_per_call_equals_batched(depth4_batched):
    """G = 1 calls: indexing by lane or by block instead of by game would show here."""
    roots = G.load()["depth4"]["roots"]
    for i in range(len(roots)):
        r = alpha_beta_search(roots[i:i + 1], max_depth=4)
        assert r.moves[0].tobytes() == depth4_batched.moves[i].tobytes() and r.scores[0] == depth4_batched.scores[i], i
        assert r.stats.positions == r.stats.max_positions_per_root > 0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65])
def test_batch_sizes_around_the_wave_and_block_width(n):
    """A block answers 4 roots (one per wave): 3, 4, 5 cross it, 63, 64, 65 the wave width. Slices start at
    an offset so root 0 of the call is not root 0 of the golden."""
    sec = G.load()["depth4"]
    lo = 37
    r = alpha_beta_search(sec["roots"][lo:lo + n], max_depth=4)
    assert len(r.moves) == n and not _mismatch(r, sec, lo, lo + n)


def test_depth5_equals_golden():
    sec = G.load()["depth6"]
    r = alpha_beta_search(sec["roots"], max_depth=6)
    assert not _mismatch(r, sec)


@pytest.mark.parametrize("max_depth", [2, 3, 5])
def test_mate_in_one_at_the_other_depths(max_depth):
    """Depths without goldens (1, 2 and 4 plies): the mate in one and its score are found at every depth."""
    d = G.load()
    hand = {h["name"]: h for h in d["hand"]}
    names = ["mate_capture_red", "mate_capture_blue", "mate_temple_red", "mate_temple_blue"]
    r = alpha_beta_search(G.states([hand[n]["state"] for n in names]), max_depth=max_depth)
    assert r.scores.tolist() == [10000, -10000, 10000, -10000]
    assert [m.tolist() for m in r.moves] == [tuple(hand[n]["move"]) for n in names]


def test_hand_built_positions():
    hand = G.load()["hand"]
    roots = G.states([h["state"] for h in hand])
    assert {h["max_depth"] for h in hand} == {4}
    r = alpha_beta_search(roots, max_depth=4)
    for i, h in enumerate(hand):
        assert list(r.moves[i].tolist()) == h["move"] and int(r.scores[i]) == h["score"], (h["name"], r.moves[i], r.scores[i])
    by = {h["name"]: i for i, h in enumerate(hand)}
    assert r.moves[by["no_move_red"]].tolist() == (25, 25, 0, 0) and r.scores[by["no_move_red"]] == G.INT32_MIN
    assert r.moves[by["no_move_blue"]].tolist() == (25, 25, 0, 2) and r.scores[by["no_move_blue"]] == G.INT32_MAX
    assert r.stats.roots_without_move == 2
    assert r.scores[by["interior_no_move_blue_root"]] == G.INT32_MIN
    assert r.scores[by["interior_no_move_red_root"]] == G.INT32_MAX


def test_stats(depth4_batched):
    st = depth4_batched.stats
    # (the counts themselves are not the restatement's: every root child is searched with the full window)
    assert st.positions > 0 and 0 < st.max_positions_per_root <= st.positions and st.roots_without_move == 0


def test_agent_generate_move_on_the_start_position():
    """Agent::generate_move (mod.rs:136-170) on the start position with Tiger, Dragon, Frog, Rabbit, Crab (Blue
    to move): the restatement's anchors, -12 at max_depth 4 and -16 at 6, both by a5 -> b4 with Frog (slot 2)."""
    gs = GameState.with_deck(Deck([ORIGINAL_CARDS[i] for i in range(5)]))
    for depth, score in ((4, -12.0), (6, -16.0)):
        mv, value = AlphaBeta(max_depth=depth).generate_move(gs)
        assert (mv.mov.from_, mv.mov.to, int(mv.mov.piece), mv.used_card_idx) == (0, 6, 0, 2)
        assert value == score and isinstance(value, float)
    sec = G.load()["depth4"]
    assert AlphaBeta(max_depth=4).generate_moves_np(sec["roots"][5:9]).tobytes() == sec["move_np"][5:9].tobytes()


def test_alphabeta_vs_alphabeta_games_equal_golden():
    """fight() with the agent on both sides: alternation, passes, the ply cut and batches that shrink as
    games end, against the restatement's games under the reference's loop (evaluator.rs:373-389)."""
    g = G.load()["games"]
    st = fight(EvaluatorConfig(game_amnt=len(g["result"]), deck=None, max_plies=g["max_plies"], seed=g["seed"]),
               AlphaBeta(g["max_depth"]), AlphaBeta(g["max_depth"]))
    assert st.results == g["result"]
    assert st.plies == g["plies"]


def test_pit_with_alphabeta_fight():
    best = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=21)
    new = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=22)
    ev = Evaluator(EvaluatorConfig(game_amnt=4, max_plies=60, seed=9), best, new)
    with_ab, promote_ab = ev.pit(sims=16, alphabeta=True, enforce_search_time=False)
    without, promote = ev.pit(sims=16, alphabeta=False, enforce_search_time=False)
    assert without.alphabeta_fight is None
    ab = with_ab.alphabeta_fight
    assert ab is not None and len(ab.results) == 4 and len(ab.plies) == 4 and len(ab.rating_change_history) == 4
    assert ab.general.wins + ab.general.loses + ab.general.draws == 4
    assert promote_ab == promote
    for a, b in ((with_ab.self_fight, without.self_fight), (with_ab.random_fight, without.random_fight),
                 (with_ab.mcts_fight, without.mcts_fight)):
        assert a.results == b.results and a.plies == b.plies
        assert (a.rating_a, a.rating_b, a.general) == (b.rating_a, b.rating_b, b.general)
