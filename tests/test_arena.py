"""The arena's host side (include/onitama_az.h, "arena"): Elo and the FightStatistics fold against the Python
mirror of evaluator.rs / elo_rating.rs, the Random agent's move (ai/random.rs:11-43) rebuilt from the oracle's
Philox and move generation, and oaz_arena_fight's argument checks, all of which run without a GPU."""
import ctypes as C
import math

import numpy as np

from conftest import random_positions
from onitama_az import _abi
from onitama_az.evaluator import EloRating, FightStatistics
from onitama_az.game import MoveResult, PlayerColor

RAND = 0x52414E44


# ---- Elo and the fold -------------------------------------------------------------------------------------
def test_elo_change_matches_python(lib):
    rng = np.random.default_rng(7)
    for ra, rb in [(800.0, 800.0), (1000.0, 800.0), (0.0, 3000.0)] + [tuple(rng.uniform(0, 3000, 2)) for _ in range(50)]:
        for won in (True, False):
            a, b = C.c_double(), C.c_double()
            lib.oaz_elo_change(ra, rb, int(won), C.byref(a), C.byref(b))
            ea, eb = EloRating.elo_change(ra, rb, won)
            assert abs(a.value - ea) <= 1e-9 and abs(b.value - eb) <= 1e-9
    a, b = C.c_double(), C.c_double()
    lib.oaz_elo_change(800.0, 800.0, 1, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (816.0, 784.0)


def _same(x, y):
    return (math.isnan(x) and math.isnan(y)) or x == y


def test_fight_stats_fold_matches_python(lib):
    rng = np.random.default_rng(20260101)
    lengths = [0, 1, 2, 37]
    for case in range(200):
        n = lengths[case % 4]
        res = rng.integers(0, 4, n).astype(np.uint8)  # all four MoveResult codes
        ra, rb = (800.0, 800.0) if case < 8 else tuple(rng.uniform(400, 1600, 2))
        ref = FightStatistics(ra, rb)
        for k, r in enumerate(res):
            ref.update(MoveResult(int(r)), PlayerColor.Red if k % 2 == 0 else PlayerColor.Blue)
        st = _abi.oaz_fight_stats()
        hist = np.full((n, 4), -1.0)
        assert lib.oaz_fight_stats_fold(_abi.ptr(res) if n else None, n, ra, rb, C.byref(st), _abi.ptr(hist) if n else None) == 0
        assert (st.wins, st.loses, st.draws) == (ref.general.wins, ref.general.loses, ref.general.draws)
        for c in (0, 1):
            assert (st.color_wins[c], st.color_loses[c], st.color_draws[c]) == (ref.color[c].wins, ref.color[c].loses,
                                                                                ref.color[c].draws)
            assert _same(st.color_winrate[c], ref.color_winrate[c]), (n, c)
        assert _same(st.winrate, ref.winrate)
        assert abs(st.rating_a - ref.rating_a) <= 1e-9 and abs(st.rating_b - ref.rating_b) <= 1e-9
        assert len(ref.rating_change_history) == n
        for k, h in enumerate(ref.rating_change_history):
            assert np.abs(hist[k] - [h.before_a, h.after_a, h.before_b, h.after_b]).max() <= 1e-9
        assert (st.plies_total, st.passes) == (0, 0)


def test_fight_stats_fold_rejects_bad_arguments(lib):
    st = _abi.oaz_fight_stats()
    bad = np.array([1, 4], dtype=np.uint8)
    assert lib.oaz_fight_stats_fold(_abi.ptr(bad), 2, 800.0, 800.0, C.byref(st), None) == _abi.ERR_ARG
    assert lib.oaz_fight_stats_fold(None, 2, 800.0, 800.0, C.byref(st), None) == _abi.ERR_ARG
    assert lib.oaz_fight_stats_fold(_abi.ptr(bad), 2, 800.0, 800.0, None, None) == _abi.ERR_ARG


# ---- Random agent -----------------------------------------------------------------------------------------
def _native_move(lib, seed, game, ply, s):
    mv = np.zeros(1, dtype=_abi.MOVE_DTYPE)
    assert lib.oaz_random_agent_move(seed, game, ply, _abi.ptr(np.ascontiguousarray(s.reshape(1))), _abi.ptr(mv)) == 0
    return tuple(int(mv[0][f]) for f in ("from_", "to", "piece", "slot"))


def _expected_move(orc, seed, game, ply, s):
    w = orc.philox(seed, (game & 0xFFFFFFFF, game >> 32, RAND, ply))
    card_idx = (int(w[0]) * 2) >> 32
    base = 0 if int(s["to_move"]) == 0 else 2
    cand = [m for m in orc.movegen(s) if int(m["slot"]) == base + card_idx]
    if not cand:
        return (0, 5, 0, card_idx)
    m = cand[(int(w[1]) * len(cand)) >> 32]
    return (int(m["from_"]), int(m["to"]), int(m["piece"]), card_idx)


def test_random_agent_move_matches_oracle_rebuild(lib, orc):
    seed = 20260419
    roots = random_positions(orc, 2000, seed=91)
    rng = np.random.default_rng(3)
    colours = set()
    for i in range(len(roots)):
        s = roots[i:i + 1].copy()
        game = int(rng.integers(0, 1 << 40)) if i % 3 == 0 else i  # (game ids past 32 bits: both counter words)
        ply = int(rng.integers(0, 152))
        for colour in (0, 1):  # both colours on every position
            s["to_move"][0] = colour
            got = _native_move(lib, seed, game, ply, s[0])
            assert got == _expected_move(orc, seed, game, ply, s[0]), (i, colour)
            assert got[3] in (0, 1)  # random.rs:39: used_card_idx is 0 / 1 for Blue too
            colours.add(colour)
    assert colours == {0, 1}


def test_random_agent_move_without_a_move_of_the_drawn_card(lib, orc):
    # Red's whole army in file a (king a5, pawns a4 a3 a2 a1) holding Tiger (two up or one down, card.rs): every
    # Tiger target is off the board or on an own piece; the second card, Crab, has moves. Blue: a king on e1.
    bit = lambda sq: 0x80000000 >> sq  # noqa: E731
    s = orc.state([bit(0), bit(24)], [bit(5) | bit(10) | bit(15) | bit(20), 0], [0, 4, 2, 3, 5], 0)
    by_slot = [[m for m in orc.movegen(s[0]) if int(m["slot"]) == k] for k in (0, 1)]
    assert not by_slot[0] and by_slot[1]
    drawn = set()
    for game in range(64):
        w = orc.philox(5, (game, 0, RAND, 9))
        card_idx = (int(w[0]) * 2) >> 32
        got = _native_move(lib, 5, game, 9, s[0])
        assert got == _expected_move(orc, 5, game, 9, s[0])
        if card_idx == 0:
            assert got == (0, 5, 0, 0)  # random.rs:27-33: a5 -> a4 with a pawn
        else:
            assert got[3] == 1 and got[:3] in {(int(m["from_"]), int(m["to"]), int(m["piece"])) for m in by_slot[1]}
        drawn.add(card_idx)
    assert drawn == {0, 1}


def test_random_agent_move_covers_both_cards_and_every_move(lib, orc):
    s = random_positions(orc, 40, seed=12)[17:18]
    legal = {(int(m["from_"]), int(m["to"]), int(m["piece"]), int(m["slot"]) - (0 if int(s["to_move"][0]) == 0 else 2))
             for m in orc.movegen(s[0])}
    assert {m[3] for m in legal} == {0, 1}
    got = {_native_move(lib, 77, game, ply, s[0]) for game in range(64) for ply in range(64)}  # 4 096 pairs
    assert got == legal


def test_random_agent_move_rejects_bad_state(lib):
    s = np.zeros(1, dtype=_abi.STATE_DTYPE)
    mv = np.zeros(1, dtype=_abi.MOVE_DTYPE)
    s["to_move"][0] = 2
    assert lib.oaz_random_agent_move(1, 0, 0, _abi.ptr(s), _abi.ptr(mv)) == _abi.ERR_ARG
    assert lib.oaz_random_agent_move(1, 0, 0, None, _abi.ptr(mv)) == _abi.ERR_ARG


# ---- oaz_arena_fight: arguments (no device is reached) ------------------------------------------------------
def _cfg(lib, **kw):
    c = _abi.oaz_arena_config()
    lib.oaz_arena_config_default(C.byref(c))
    for k, v in kw.items():
        if k == "deck":
            c.fixed_deck = 1
            for i, card in enumerate(v):
                c.deck[i] = card
        else:
            setattr(c, k, v)
    return c


def _agent(kind, engine=None, max_depth=4):
    a = _abi.oaz_arena_agent()
    a.kind, a.engine = kind, engine
    a.alphabeta.max_depth = max_depth
    a.mcts.max_playouts, a.mcts.min_node_visits, a.mcts.rollout_cap, a.mcts.exploration_c = 50, 5, 1000, 1.41
    return a


def _fight(lib, cfg, a, b, stats=True):
    st = _abi.oaz_fight_stats()
    rc = lib.oaz_arena_fight(C.byref(cfg) if cfg is not None else None, C.byref(a) if a is not None else None,
                             C.byref(b) if b is not None else None, 800.0, 800.0, C.byref(st) if stats else None,
                             None, None, None)
    return rc, st, lib.oaz_last_error().decode()


def test_arena_config_default(lib):
    c = _cfg(lib)
    assert (c.game_amnt, c.max_plies, c.fixed_deck, c.device) == (20, 150, 0, 0)  # evaluator.rs:129-136


def test_arena_capacity(lib, orc):
    out = (C.c_int32 * 2)()
    assert lib.oaz_arena_capacity(C.byref(_cfg(lib, game_amnt=7, deck=[0, 1, 2, 3, 4])), C.byref(out)) == 0
    assert tuple(out) == (4, 4)  # a fixed deck: every game has the same first mover
    c = _cfg(lib, game_amnt=33, seed=5)
    assert lib.oaz_arena_capacity(C.byref(c), C.byref(out)) == 0
    first = sum((int(orc.initial_state(orc.deal_deck(5, k))["to_move"][0]) == 0) == (k % 2 == 0) for k in range(33))
    assert tuple(out) == (max(first, 33 - first),) * 2
    assert lib.oaz_arena_capacity(C.byref(_cfg(lib, game_amnt=0)), C.byref(out)) == 0 and tuple(out) == (0, 0)


def test_arena_fight_argument_errors(lib):
    rnd, ab = _agent(_abi.AGENT_RANDOM), _agent(_abi.AGENT_ALPHABETA)
    cases = [
        (None, rnd, rnd, True),                                             # null config
        (_cfg(lib), None, rnd, True),                                       # null agent
        (_cfg(lib), rnd, None, True),                                       # null opponent
        (_cfg(lib), rnd, rnd, False),                                       # null stats
        (_cfg(lib, game_amnt=-1), rnd, rnd, True),
        (_cfg(lib), _agent(7), rnd, True),                                  # unknown kind
        (_cfg(lib), rnd, _agent(-1), True),
        (_cfg(lib), _agent(_abi.AGENT_ALPHAZERO), rnd, True),               # no engine
        (_cfg(lib, deck=[0, 1, 2, 3, 16]), rnd, rnd, True),                 # card >= 16
        (_cfg(lib, deck=[0, 1, 2, 1, 4]), rnd, rnd, True),                  # repeated card
        (_cfg(lib), rnd, _agent(_abi.AGENT_ALPHABETA, max_depth=1), True),  # max_depth outside 2..6
        (_cfg(lib), _agent(_abi.AGENT_ALPHABETA, max_depth=7), rnd, True),
    ]
    for cfg, a, b, stats in cases:
        rc, _, msg = _fight(lib, cfg, a, b, stats)
        assert rc == _abi.ERR_ARG and msg, (rc, msg)
    # the same checks come before the device is looked for when nothing is wrong with the rest
    rc, _, msg = _fight(lib, _cfg(lib, game_amnt=0, deck=[5, 5, 1, 2, 3]), rnd, ab)
    assert rc == _abi.ERR_ARG and "repeats" in msg


def test_arena_fight_zero_games_is_ok_without_a_device(lib):
    for a, b in ((_agent(_abi.AGENT_RANDOM), _agent(_abi.AGENT_ALPHABETA)),
                 (_agent(_abi.AGENT_PURE_MCTS), _agent(_abi.AGENT_RANDOM))):
        st = _abi.oaz_fight_stats()
        st.wins = 9
        rc = lib.oaz_arena_fight(C.byref(_cfg(lib, game_amnt=0)), C.byref(a), C.byref(b), 812.5, 790.0, C.byref(st),
                                 None, None, None)
        assert rc == 0
        assert (st.rating_a, st.rating_b, st.wins, st.loses, st.draws, st.plies_total, st.passes) == (812.5, 790.0, 0, 0,
                                                                                                      0, 0, 0)
        assert st.winrate == 0.0 and list(st.color_winrate) == [0.0, 0.0]


def test_arena_start_positions_are_checked(lib, orc):
    good = orc.initial_state([0, 1, 2, 3, 4])
    bad = good.copy()
    bad["cards"][0][2] = 16
    starts = np.concatenate([good, bad])
    cfg = _cfg(lib, game_amnt=2)
    cfg.start = starts.ctypes.data
    rc, _, msg = _fight(lib, cfg, _agent(_abi.AGENT_RANDOM), _agent(_abi.AGENT_RANDOM))
    assert rc == _abi.ERR_ARG and "start position 1" in msg
    out = (C.c_int32 * 2)()
    cfg.game_amnt = 1  # only the good one (either side may move first: the capacity covers both)
    assert lib.oaz_arena_capacity(C.byref(cfg), C.byref(out)) == 0 and tuple(out) == (1, 1)
