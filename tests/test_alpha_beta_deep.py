"""CPU: the host side of the split alpha-beta search (oaz_alphabeta_generate_move) and of the tournament
(onitama_az/tournament.py, bin/tournament.rs): the ABI's structs, defaults and argument checks, the Python
mirror's defaults, the deep goldens' freshness and shape, the Elo fold and the pairing order. No GPU compute is
called here."""
import ctypes as C
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import alphabeta_deep_golden as D
import alphabeta_golden as G
from onitama_az import _abi
from onitama_az.alpha_beta import AlphaBeta
from onitama_az.tournament import AGENTS, PAIRINGS, Tournament, fold_pairing

ROOT = Path(__file__).resolve().parents[1]


def _call(lib, roots, n, cfg, stats=None, mv=True, sc=True):
    moves = np.zeros(max(n, 1), dtype=_abi.MOVE_DTYPE)
    scores = np.zeros(max(n, 1), dtype=np.int32)
    return lib.oaz_alphabeta_generate_move(None if roots is None else _abi.ptr(roots), n, cfg,
                                           _abi.ptr(moves) if mv else None, _abi.ptr(scores) if sc else None, stats)


def _cfg(lib, **kw):
    cfg = _abi.oaz_alphabeta_agent_config()
    lib.oaz_alphabeta_agent_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_struct_layout_and_default_config(lib):
    c, s = _abi.oaz_alphabeta_agent_config, _abi.oaz_alphabeta_agent_stats
    assert C.sizeof(c) == 32
    assert [(getattr(c, f).offset) for f in ("max_depth", "device", "search_time_ns", "split", "reserved")] == [0, 4, 8, 16, 20]
    assert C.sizeof(s) == 56
    assert [getattr(s, f).offset for f in ("positions", "max_positions_per_root", "roots_without_move", "items",
                                           "iterations", "plies", "split", "reserved", "elapsed_ms")] == [
        0, 8, 16, 24, 32, 36, 40, 44, 48]
    cfg = _abi.oaz_alphabeta_agent_config()
    cfg.max_depth, cfg.device, cfg.search_time_ns, cfg.split = -1, 9, 7, 2
    lib.oaz_alphabeta_agent_config_default(C.byref(cfg))
    assert (cfg.max_depth, cfg.device, cfg.search_time_ns, cfg.split) == (6, 0, 1_000_000_000, 0)  # mod.rs:21-28
    # the existing structs and the ABI version are what they were
    assert C.sizeof(_abi.oaz_alphabeta_config) == 16 and C.sizeof(_abi.oaz_alphabeta_stats) == 24
    assert lib.oaz_abi_version() == 5


@pytest.mark.parametrize("field, value, word", [
    ("max_depth", 1, b"max_depth"), ("max_depth", 9, b"max_depth"), ("max_depth", 0, b"max_depth"),
    ("max_depth", -3, b"max_depth"), ("split", -1, b"split"), ("split", 4, b"split"),
    ("search_time_ns", -1, b"search_time_ns"),
])
def test_generate_move_rejects_bad_config_before_any_device(lib, field, value, word):
    """Checked before device selection (here also with a device number that cannot exist), so the answer is
    OAZ_ERR_ARG with or without a GPU."""
    roots = G.load()["depth4"]["roots"][:2].copy()
    for device in (0, 1 << 20):
        cfg = _cfg(lib, device=device, **{field: value})
        assert _call(lib, roots, 2, C.byref(cfg)) == _abi.ERR_ARG
        assert word in lib.oaz_last_error()


def test_generate_move_rejects_null_pointers_and_invalid_roots(lib):
    cfg = _cfg(lib)
    roots = G.load()["depth4"]["roots"][:1].copy()
    assert _call(lib, None, 1, C.byref(cfg)) == _abi.ERR_ARG
    assert _call(lib, roots, 1, None) == _abi.ERR_ARG
    assert _call(lib, roots, 1, C.byref(cfg), mv=False) == _abi.ERR_ARG
    assert _call(lib, roots, 1, C.byref(cfg), sc=False) == _abi.ERR_ARG
    assert _call(lib, roots, -1, C.byref(cfg)) == _abi.ERR_ARG
    assert b"null" in lib.oaz_last_error()
    for field, value in (("pawns", (0x40, 0)), ("kings", (0, 1)), ("cards", (0, 1, 2, 3, 16)), ("to_move", 2)):
        bad = roots.copy()
        bad[field][0] = value
        assert _call(lib, bad, 1, C.byref(cfg)) == _abi.ERR_ARG, field
        assert b"root 0" in lib.oaz_last_error()
    # max_depth 7 and 8 pass the argument checks (the answer is then the device's, or OAZ_ERR_NO_DEVICE), while
    # the old entry point still rejects 7 (tests/test_alpha_beta.py pins that)
    old = _abi.oaz_alphabeta_config()
    lib.oaz_alphabeta_config_default(C.byref(old))
    old.max_depth = 7
    mv, sc = np.zeros(1, dtype=_abi.MOVE_DTYPE), np.zeros(1, dtype=np.int32)
    assert lib.oaz_alphabeta_search(_abi.ptr(roots), 1, C.byref(old), _abi.ptr(mv), _abi.ptr(sc), None) == _abi.ERR_ARG


def test_header_and_exported_symbols_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "onitama_az.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(oaz_[a-z0-9_]+)\s*\(", text))
    assert {"oaz_alphabeta_generate_move", "oaz_alphabeta_agent_config_default"} <= names
    assert names == set(_abi.EXPORTED_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n


def test_python_mirror_defaults_and_id():
    ab = AlphaBeta()
    assert (ab.max_depth, ab.search_time, ab.device, ab.enforce_search_time, ab.split) == (6, 1.0, 0, False, 0)
    assert not ab._deep() and not AlphaBeta(max_depth=4, search_time=0.4)._deep()  # the path they had
    assert ab.id() == 1_000_000_000 + 6 and ab.name() == "AlphaBeta AI"
    deep = AlphaBeta(max_depth=8)  # tournament.rs:107-110
    assert deep._deep() and deep.id() == 1_000_000_000 + 8
    assert AlphaBeta(max_depth=7)._deep() and AlphaBeta(enforce_search_time=True)._deep()
    import onitama_az
    assert onitama_az.Tournament is Tournament and callable(onitama_az.alpha_beta_generate_move)


def test_deep_golden_is_fresh(tmp_path, orc):
    """The committed golden equals what the restatement, compiled now, writes for the same seeds."""
    sys.path.insert(0, str(ROOT / "tools"))
    import make_alphabeta_deep_kats as gen
    ref = gen.base.build_ref(tmp_path)
    if ref is None:
        pytest.skip("no C compiler")
    assert gen.base.dumps(gen.generate(ref)) == D.PATH.read_text()


def test_deep_golden_shape():
    d = D.load()
    assert len(d["depth7"]["states"]) == 16 and d["depth7"]["max_depth"] == 7
    assert len(d["depth8"]["states"]) == 4 and d["depth8"]["max_depth"] == 8
    assert max(d["depth8"]["positions"]) < 17_000_000  # under a second at the restatement's 17.7 M positions/s
    assert len(d["hand"]) == 8 and all(h["max_depth"] == [3, 4, 5, 6, 7, 8] for h in d["hand"])
    hand = {h["name"]: h for h in d["hand"]}
    assert set(hand) == {h["name"] for h in G.load()["hand"]}
    for h in G.load()["hand"]:  # the same positions, and at max_depth 4 the same answers
        deep = hand[h["name"]]
        assert deep["state"] == h["state"] and deep["move"][1] == h["move"] and deep["score"][1] == h["score"]
    assert hand["no_move_red"]["score"] == [G.INT32_MIN] * 6 and hand["no_move_blue"]["score"] == [G.INT32_MAX] * 6
    assert all(n > 0 for n in hand["interior_no_move_blue_root"]["interior_without_move"])
    assert all(n > 0 for n in hand["interior_no_move_red_root"]["interior_without_move"])
    g = d["games"]
    assert (g["max_depth"], g["max_plies"], len(g["result"])) == (7, 30, 2)
    assert all(len(m) == p <= 30 for m, p in zip(g["moves"], g["plies"]))
    assert D.PATH.stat().st_size < 200_000


# ---- the tournament's fold and order -------------------------------------------------------------------------
def _elo(lib, ra, rb, a_won):
    a, b = C.c_double(), C.c_double()
    lib.oaz_elo_change(ra, rb, int(a_won), C.byref(a), C.byref(b))
    return a.value, b.value


def test_fold_pairing_against_hand_computed_chains(lib):
    R, B, CUT = _abi.RED_WIN, _abi.BLUE_WIN, _abi.IN_PROGRESS
    # game 0 (first-named is Red): Red wins -> a win; game 1 (it is Blue): Red wins -> a loss; game 2: cut by the
    # ply budget -> nothing; game 3 (Blue): Blue wins -> a win
    ra, rb = _elo(lib, 800.0, 800.0, True)
    assert (ra, rb) == (816.0, 784.0)  # K = 32, equal ratings: +-16
    ra, rb = _elo(lib, ra, rb, False)
    ra, rb = _elo(lib, ra, rb, True)
    assert fold_pairing([R, R, CUT, B], 800.0, 800.0) == (ra, rb, 2, 1)
    # a capture as the last result is no result either (tournament.rs:62), and ratings are carried in
    assert fold_pairing([_abi.CAPTURE, CUT], 812.5, 790.25) == (812.5, 790.25, 0, 2)
    assert fold_pairing([], 801.0, 799.0) == (801.0, 799.0, 0, 0)
    a2, b2 = _elo(lib, 812.5, 790.25, False)
    assert fold_pairing([B], 812.5, 790.25) == (a2, b2, 0, 0)


class _Stub:
    def __init__(self, name):
        self._name = name

    def name(self):
        return self._name


def test_tournament_pairing_order_decks_and_rating_chain(lib, capsys):
    assert [(AGENTS[i], AGENTS[j]) for i, j in PAIRINGS] == [  # tournament.rs:136-188
        ("alphabeta", "mcts"), ("alphabeta", "alphazero"), ("alphabeta", "random"), ("mcts", "alphazero"),
        ("mcts", "random"), ("alphazero", "random")]
    R, B, CUT = _abi.RED_WIN, _abi.BLUE_WIN, _abi.IN_PROGRESS
    script = [[R, R, B], [R, CUT, B], [B, B, B], [CUT, CUT, CUT], [R, B, R], [B, R, CUT]]
    calls = []

    def play(config, agent, opponent, *ratings):
        assert ratings == ()  # the fight's own Elo is not the tournament's
        calls.append((agent.name(), opponent.name(), config.game_amnt, config.max_plies, config.seed, config.deck))
        return SimpleNamespace(results=script[len(calls) - 1], plies=[5, 6, 7])

    agents = [_Stub(n) for n in ("AB", "MC", "AZ", "RN")]
    t = Tournament(*agents, game_amnt=3, max_plies=40, seed=77, play=play)
    out = t.pit()
    assert [c[:2] for c in calls] == [("AB", "MC"), ("AB", "AZ"), ("AB", "RN"), ("MC", "AZ"), ("MC", "RN"), ("AZ", "RN")]
    assert all(c[2:] == (3, 40, 77, None) for c in calls)  # every pairing deals oaz_deal_deck(77, k)
    decks = []
    for k in range(3):
        d = (C.c_uint8 * 5)()
        lib.oaz_deal_deck(77, k, d)
        decks.append(list(d))
    assert t.decks == decks and all(p.decks == decks for p in out)
    # the ratings are chained through the pairings, the fold as fold_pairing's
    r = {k: 800.0 for k in AGENTS}
    for (i, j), res, p in zip(PAIRINGS, script, out):
        a, b = AGENTS[i], AGENTS[j]
        r[a], r[b], wins, cut = fold_pairing(res, r[a], r[b])
        assert (p.agent, p.opponent, p.results, p.plies, p.wins, p.cut) == (a, b, res, [5, 6, 7], wins, cut)
        assert p.ratings == r and p.winrate == wins / 3 and p.elapsed_s >= 0
    assert out[3].ratings == out[2].ratings  # three cut games change nothing
    assert out[0].wins == 1 and out[2].cut == 0 and out[3].cut == 3 and t.ratings == r
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == f"AB ({out[0].ratings['alphabeta']:5.2f}) vs MC ({out[0].ratings['mcts']:5.2f}) -> winrate: 0.33"
    assert lines[1].startswith("Elapsed: ") and len([x for x in lines if x.startswith("Elapsed")]) == 6
