"""CPU: the alpha-beta agent's host side (onitama-game/src/ai/alpha_beta/): the static evaluation
through the C ABI against the CPU restatement's goldens (tests/c/alphabeta_ref.c ->
tests/golden/alphabeta_kats.json), the golden's freshness, the ABI's defaults and argument checks and
the Python mirror. No GPU compute is called here."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import alphabeta_golden as G
from onitama_az import _abi
from onitama_az.alpha_beta import AlphaBeta, alpha_beta_evaluate
from onitama_az.evaluator import FightStatistics, PitStatistics

ROOT = Path(__file__).resolve().parents[1]


def test_evaluate_equals_golden():
    """oaz_alphabeta_evaluate on the 512 (state, move_result) cases: None through the NULL pointer, the four
    MoveResult values through the array."""
    ev = G.load()["evaluate"]
    s = G.states(ev["states"])
    mr = np.array(ev["move_result"], dtype=np.uint8)
    want = np.array(ev["value"], dtype=np.int32)
    assert len(s) == 512 and set(mr.tolist()) == {G.NONE, 0, 1, 2, 3}
    none = mr == G.NONE
    got = np.zeros(len(s), dtype=np.int32)
    got[none] = alpha_beta_evaluate(s[none], None)
    got[~none] = alpha_beta_evaluate(s[~none], mr[~none])
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]]
    # the cases are not degenerate: both colours, won results, positions without a king (get_msb = 0)
    assert {int(x) for x in s["to_move"]} == {0, 1}
    assert (np.abs(want) == 10000).sum() > 100 and (np.abs(want) != 10000).sum() > 200
    assert ((s["kings"] == 0).any(axis=1) & ~np.isin(mr, (1, 2))).any()


def test_evaluate_hand_derived_anchors(lib):
    """The start position with Tiger, Dragon, Frog, Rabbit, Crab, derived by hand from evaluation.rs: temple,
    piece and piece-square terms cancel; closeness is 12 - 20 for Red to move and -(20 - 12) for Blue."""
    d = (C.c_uint8 * 5)(0, 1, 2, 3, 4)
    s = np.zeros(2, dtype=_abi.STATE_DTYPE)
    lib.oaz_initial_state(d, _abi.ptr(s[0:1]))
    s[1] = s[0]
    s["to_move"] = (0, 1)
    assert alpha_beta_evaluate(s).tolist() == [-8, -8]


def test_evaluate_rejects_bad_arguments(lib):
    s = np.zeros(1, dtype=_abi.STATE_DTYPE)
    out = np.zeros(1, dtype=np.int32)
    mr = np.array([4], dtype=np.uint8)
    assert lib.oaz_alphabeta_evaluate(_abi.ptr(s), _abi.ptr(mr), 1, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_alphabeta_evaluate(None, None, 1, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_alphabeta_evaluate(None, None, 0, None) == 0


def test_golden_is_fresh(tmp_path, orc):
    """The committed golden equals what the restatement, compiled now, writes for the same seeds."""
    sys.path.insert(0, str(ROOT / "tools"))
    import make_alphabeta_kats as gen
    ref = gen.build_ref(tmp_path)
    if ref is None:
        pytest.skip("no C compiler")
    assert gen.dumps(gen.generate(ref)) == G.PATH.read_text()


def test_golden_anchors_of_the_restatement(tmp_path, orc):
    """The restatement against the figures a scratch prototype gave for the start position (Tiger, Dragon,
    Frog, Rabbit, Crab; Blue to move): max_depth 4 -> -12, 0->6 pawn slot 2, 401 positions; max_depth 6 ->
    -16, the same move, 29 329 positions."""
    sys.path.insert(0, str(ROOT / "tools"))
    import make_alphabeta_kats as gen
    ref = gen.build_ref(tmp_path)
    if ref is None:
        pytest.skip("no C compiler")
    root = orc.initial_state([0, 1, 2, 3, 4])
    assert int(root["to_move"][0]) == 1
    assert gen.ref_search(ref, root[0], 4)[:3] == ((0, 6, 0, 2), -12, 401)
    assert gen.ref_search(ref, root[0], 6)[:3] == ((0, 6, 0, 2), -16, 29329)


def test_golden_shape():
    d = G.load()
    assert len(d["depth4"]["states"]) == 256 and d["depth4"]["max_depth"] == 4
    assert len(d["depth6"]["states"]) == 32 and d["depth6"]["max_depth"] == 6
    assert len(d["games"]["result"]) == 8 and all(len(m) == p for m, p in zip(d["games"]["moves"], d["games"]["plies"]))
    hand = {h["name"]: h for h in d["hand"]}
    assert hand["no_move_red"]["move"] == [25, 25, 0, 0] and hand["no_move_red"]["score"] == G.INT32_MIN
    assert hand["no_move_blue"]["move"] == [25, 25, 0, 2] and hand["no_move_blue"]["score"] == G.INT32_MAX
    assert hand["interior_no_move_blue_root"]["interior_without_move"] > 0
    assert hand["interior_no_move_blue_root"]["score"] == G.INT32_MIN
    assert hand["interior_no_move_red_root"]["interior_without_move"] > 0
    assert hand["interior_no_move_red_root"]["score"] == G.INT32_MAX
    assert [hand[f"mate_{k}_{c}"]["score"] for k in ("capture", "temple") for c in ("red", "blue")] == [
        10000, -10000, 10000, -10000]
    assert G.PATH.stat().st_size < 200_000


def test_config_default(lib):  # alpha_beta/mod.rs:21-28
    cfg = _abi.oaz_alphabeta_config()
    cfg.max_depth, cfg.device = -1, 9
    lib.oaz_alphabeta_config_default(C.byref(cfg))
    assert (cfg.max_depth, cfg.device) == (6, 0)
    assert C.sizeof(_abi.oaz_alphabeta_config) == 16 and C.sizeof(_abi.oaz_alphabeta_stats) == 24


@pytest.mark.parametrize("max_depth", [1, 7, 0, -3])
def test_search_rejects_max_depth_before_any_device(lib, max_depth):
    """max_depth < 2 panics in the reference (mod.rs:161); above 6 is not opened. Checked before device
    selection, so the answer is OAZ_ERR_ARG with or without a GPU."""
    roots = G.load()["depth4"]["roots"][:2].copy()
    cfg = _abi.oaz_alphabeta_config()
    lib.oaz_alphabeta_config_default(C.byref(cfg))
    cfg.max_depth = max_depth
    mv = np.zeros(2, dtype=_abi.MOVE_DTYPE)
    sc = np.zeros(2, dtype=np.int32)
    rc = lib.oaz_alphabeta_search(_abi.ptr(roots), 2, C.byref(cfg), _abi.ptr(mv), _abi.ptr(sc), None)
    assert rc == _abi.ERR_ARG
    assert b"max_depth" in lib.oaz_last_error()


def test_search_rejects_invalid_roots_before_any_device(lib):
    """A bitboard with a bit below square 24, a card id above 15 or a to_move above 1 is OAZ_ERR_ARG (the kernel
    indexes the attack table by square and card)."""
    cfg = _abi.oaz_alphabeta_config()
    lib.oaz_alphabeta_config_default(C.byref(cfg))
    mv = np.zeros(1, dtype=_abi.MOVE_DTYPE)
    sc = np.zeros(1, dtype=np.int32)
    for field, value in (("pawns", (0x40, 0)), ("kings", (0, 1)), ("cards", (0, 1, 2, 3, 16)), ("to_move", 2)):
        root = G.load()["depth4"]["roots"][:1].copy()
        root[field][0] = value
        assert lib.oaz_alphabeta_search(_abi.ptr(root), 1, C.byref(cfg), _abi.ptr(mv), _abi.ptr(sc), None) == _abi.ERR_ARG, field
    assert lib.oaz_alphabeta_search(None, 1, C.byref(cfg), _abi.ptr(mv), _abi.ptr(sc), None) == _abi.ERR_ARG
    assert lib.oaz_alphabeta_search(None, 0, None, None, None, None) == _abi.ERR_ARG  # no config


def test_python_mirror_name_and_id():  # mod.rs:172-182
    import onitama_az
    assert onitama_az.AlphaBeta is AlphaBeta
    ab = AlphaBeta()
    assert (ab.max_depth, ab.search_time, ab.device) == (6, 1.0, 0)
    assert ab.name() == "AlphaBeta AI"
    assert ab.id() == 1_000_000_000 + 6
    assert AlphaBeta(max_depth=4, search_time=0.4).id() == 400_000_000 + 4  # the arena's opponent
    assert ab.device_key() == ("alpha_beta", id(ab)) and ab.device_key() != AlphaBeta().device_key()


def test_pit_statistics_keeps_its_shape():
    st = PitStatistics(self_fight=FightStatistics())
    assert st.alphabeta_fight is None and st.random_fight is None and st.mcts_fight is None
    st = PitStatistics(FightStatistics(), FightStatistics(), FightStatistics())
    assert st.alphabeta_fight is None
