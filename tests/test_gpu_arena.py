"""The arena's fight on the device (oaz_arena_fight, arena.native_fight) against `evaluator.fight`, which is
itself tested against the oracle-driven sequential loop (tests/test_evaluator.py), and, for the Random agent
and passes, against that sequential loop restated for the HASH evaluator (tests/arena_util.py)."""
import ctypes as C
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from arena_util import C_PUCT, sequential_hash_vs_random
from onitama_az import _abi
from onitama_az.alpha_beta import AlphaBeta
from onitama_az.arena import NativeRandomAgent, arena_capacity, arena_config, native_fight
from onitama_az.engine import Engine
from onitama_az.evaluator import AlphaZeroAgent, Evaluator, EvaluatorConfig, fight
from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNet, ConvResNetConfig
from onitama_az.pure_mcts import Mcts

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _net(seed):
    return ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=seed)


@pytest.fixture(scope="module")
def nets():
    return _net(11), _net(12)


def _mcfg(sims):
    return AlphaZeroMctsConfig(exploration_c=C_PUCT, max_playouts=sims, train=False, enforce_search_time=False)


def _assert_same(nat, ref):
    assert nat.results == ref.results and nat.plies == ref.plies
    assert (nat.general, nat.color) == (ref.general, ref.color)
    assert abs(nat.rating_a - ref.rating_a) <= 1e-9 and abs(nat.rating_b - ref.rating_b) <= 1e-9
    same = lambda x, y: (x != x and y != y) or x == y  # noqa: E731 (NaN for a colour without games)
    assert same(nat.winrate, ref.winrate) and all(same(x, y) for x, y in zip(nat.color_winrate, ref.color_winrate))
    assert len(nat.rating_change_history) == len(ref.rating_change_history)
    for a, b in zip(nat.rating_change_history, ref.rating_change_history):
        assert max(abs(a.before_a - b.before_a), abs(a.after_a - b.after_a), abs(a.before_b - b.before_b),
                   abs(a.after_b - b.after_b)) <= 1e-9
    assert nat.plies_total == sum(ref.plies)


# ---- AlphaZero vs AlphaZero --------------------------------------------------------------------------------
@pytest.mark.parametrize("game_amnt", [1, 2, 5, 64, 65])
def test_alphazero_fight_equals_python_fight(nets, game_amnt):
    cfg = EvaluatorConfig(game_amnt=game_amnt, max_plies=40, seed=5)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(24), nets[0]), AlphaZeroAgent(_mcfg(24), nets[1]), 812.0, 790.0)
    ref = fight(cfg, AlphaZeroAgent(_mcfg(24), nets[0]), AlphaZeroAgent(_mcfg(24), nets[1]), 812.0, 790.0)
    _assert_same(nat, ref)


def test_one_model_on_both_sides_shares_the_engine(nets):
    cfg = EvaluatorConfig(game_amnt=5, max_plies=40, seed=6)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(24), nets[0]), AlphaZeroAgent(_mcfg(24), nets[0]))
    ref = fight(cfg, AlphaZeroAgent(_mcfg(24), nets[0]), AlphaZeroAgent(_mcfg(24), nets[0]))
    _assert_same(nat, ref)


@pytest.mark.parametrize("game_amnt", [1025, 2049])
def test_routing_past_one_scan_block(nets, game_amnt):
    """More games than the router's 1 024 threads, an odd count, random deals (so the first movers differ) and
    games ending at different plies: every ply's compaction is ragged."""
    cfg = EvaluatorConfig(game_amnt=game_amnt, max_plies=150, seed=7)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(2), nets[0]), AlphaZeroAgent(_mcfg(2), nets[1]))
    ref = fight(cfg, AlphaZeroAgent(_mcfg(2), nets[0]), AlphaZeroAgent(_mcfg(2), nets[1]))
    assert len(set(ref.plies)) > 8  # (the games do end at different plies)
    _assert_same(nat, ref)


@pytest.mark.parametrize("max_plies,cut_len", [(150, 152), (0, 2), (-1, 1)])
def test_ply_budget(nets, max_plies, cut_len):
    cfg = EvaluatorConfig(game_amnt=6, max_plies=max_plies, seed=8)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(2), nets[0]), AlphaZeroAgent(_mcfg(2), nets[1]))
    ref = fight(cfg, AlphaZeroAgent(_mcfg(2), nets[0]), AlphaZeroAgent(_mcfg(2), nets[1]))
    _assert_same(nat, ref)
    for r, n in zip(nat.results, nat.plies):
        assert n <= cut_len and ((r in (1, 2)) or n == cut_len)  # evaluator.rs:376-389
    if max_plies <= 0:
        assert nat.plies == [cut_len] * 6 and all(r not in (1, 2) for r in nat.results)


# ---- the other opponents ---------------------------------------------------------------------------------------
def test_pure_mcts_opponent_equals_python_fight(nets):
    """Pins the stream rule (game_id0 = c << 20 for the side's c-th search) and the ascending compaction order."""
    cfg = EvaluatorConfig(game_amnt=8, max_plies=60, seed=9)
    mk = lambda: Mcts(search_time=0.4, min_node_visits=5, exploration_c=1.41, max_playouts=50, seed=31)  # noqa: E731
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), mk())
    ref = fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), mk())
    _assert_same(nat, ref)
    # and with the pure-MCTS agent as the agent (side 0)
    nat = native_fight(cfg, mk(), AlphaZeroAgent(_mcfg(16), nets[1]))
    ref = fight(cfg, mk(), AlphaZeroAgent(_mcfg(16), nets[1]))
    _assert_same(nat, ref)


@pytest.mark.parametrize("max_depth", [4, 3])
def test_alphabeta_opponent_equals_python_fight(nets, max_depth):
    cfg = EvaluatorConfig(game_amnt=8, max_plies=60, seed=10)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), AlphaBeta(max_depth=max_depth))
    ref = fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), AlphaBeta(max_depth=max_depth))
    _assert_same(nat, ref)


# ---- the Random agent and passes: the C entry point against the sequential host loop ------------------------------
def _hash_fight(lib, cfg, sims, random_seed, games=None):
    need = arena_capacity(cfg)
    with Engine(games=max(games if games is not None else need[0], 1), sims=sims, c_puct=C_PUCT, train_noise=0,
                evaluator=_abi.EVAL_HASH, blocks=0) as eng:
        a, b = _abi.oaz_arena_agent(), _abi.oaz_arena_agent()
        a.kind, a.engine = _abi.AGENT_ALPHAZERO, eng.handle
        b.kind, b.seed = _abi.AGENT_RANDOM, random_seed
        n = cfg.game_amnt
        st = _abi.oaz_fight_stats()
        results, plies, hist = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, 4))
        rc = lib.oaz_arena_fight(C.byref(cfg), C.byref(a), C.byref(b), 800.0, 800.0, C.byref(st), _abi.ptr(results),
                                 _abi.ptr(plies), _abi.ptr(hist))
        return rc, st, [int(r) for r in results], [int(p) for p in plies]


def test_random_opponent_equals_sequential_host_loop(lib, orc):
    deal_seed, random_seed = 5, 77
    ref_results, ref_plies, ref_passes, quirk_games = sequential_hash_vs_random(orc, lib, 12, 60, deal_seed, random_seed, 16)
    assert quirk_games >= 2  # Blue Random movers whose used_card_idx 0 / 1 shaped the rest of their games
    rc, st, results, plies = _hash_fight(lib, arena_config(EvaluatorConfig(game_amnt=12, max_plies=60, seed=deal_seed)),
                                         16, random_seed)
    assert rc == 0, lib.oaz_last_error()
    assert (results, plies) == (ref_results, ref_plies)
    assert (st.passes, st.plies_total) == (ref_passes, sum(ref_plies))


def test_passes_equal_sequential_host_loop(lib, orc):
    """No position without a legal move turned up in 48 000 seeded HASH-vs-Random games from the deal, so the
    fight starts from one (oaz_arena_config.start): Red's army in file a (king a5, pawns a4..a1) holding Tiger and
    Horse has no move. In the even games the agent (Red) passes at ply 0; in the odd ones Random (Red) plays its
    imitation move. The reference is the sequential host loop, not the Python fight, which always deals."""
    bit = lambda sq: 0x80000000 >> sq  # noqa: E731
    stuck = orc.state([bit(0), bit(24)], [bit(5) | bit(10) | bit(15) | bit(20), bit(9) | bit(19)], [0, 11, 2, 3, 5], 0)
    assert len(orc.movegen(stuck[0])) == 0
    starts = np.concatenate([stuck] * 4)
    ref_results, ref_plies, ref_passes, _ = sequential_hash_vs_random(orc, lib, 4, 60, 0, 13, 16, starts=starts)
    assert ref_passes >= 2
    cfg = arena_config(EvaluatorConfig(game_amnt=4, max_plies=60))
    cfg.start = starts.ctypes.data
    rc, st, results, plies = _hash_fight(lib, cfg, 16, 13)
    assert rc == 0, lib.oaz_last_error()
    assert (results, plies, st.passes) == (ref_results, ref_plies, ref_passes)


def test_engine_argument_errors(lib):
    cfg = arena_config(EvaluatorConfig(game_amnt=12, max_plies=60, seed=5))
    need = arena_capacity(cfg)[0]
    rc, _, _, _ = _hash_fight(lib, cfg, 4, 1, games=need - 1)  # the engine is too small for the fight's batches
    assert rc == _abi.ERR_CAPACITY and lib.oaz_last_error()
    cfg.device = 1  # the engine is on device 0 (checked before the device number itself)
    rc, _, _, _ = _hash_fight(lib, cfg, 4, 1, games=need)
    assert rc == _abi.ERR_ARG and b"device" in lib.oaz_last_error()


# ---- pit, threads, plain C -----------------------------------------------------------------------------------------
def test_pit_native_equals_pit():
    best, new = _net(21), _net(22)
    config = EvaluatorConfig(game_amnt=4, max_plies=60, seed=9)
    ratings = ((800.0, 800.0), (820.0, 700.0), (800.0, 900.0), (810.0, 805.0))
    ev = Evaluator(config, best, new, ratings)
    nat, promote_nat = ev.pit(sims=16, alphabeta=True, enforce_search_time=False, native=True)
    ref, promote_ref = ev.pit(sims=16, alphabeta=True, enforce_search_time=False)
    assert promote_nat == promote_ref
    for a, b in ((nat.self_fight, ref.self_fight), (nat.mcts_fight, ref.mcts_fight), (nat.alphabeta_fight, ref.alphabeta_fight)):
        _assert_same(a, b)
    assert len(nat.random_fight.results) == 4
    mcfg = AlphaZeroMctsConfig(search_time=0.4, max_playouts=16, train=False, enforce_search_time=False)
    direct = native_fight(config, AlphaZeroAgent(mcfg, _net(22)), NativeRandomAgent(config.seed), *ratings[1])
    _assert_same(nat.random_fight, direct)


def test_two_fights_on_two_threads_equal_one_after_the_other(nets):
    cfg = EvaluatorConfig(game_amnt=9, max_plies=40, seed=12)
    third = _net(13)
    jobs = [lambda: native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), AlphaZeroAgent(_mcfg(16), nets[1])),
            lambda: native_fight(cfg, AlphaZeroAgent(_mcfg(16), third), NativeRandomAgent(4))]
    one_by_one = [j() for j in jobs]
    with ThreadPoolExecutor(max_workers=2) as pool:
        together = [f.result() for f in [pool.submit(j) for j in jobs]]
    for a, b in zip(together, one_by_one):
        _assert_same(a, b)


def test_arena_from_plain_c(lib, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "arena_smoke"
    lib_dir = _abi.LIB_PATH.parent
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib"
    subprocess.run([cc, "-O1", "-Wall", "-o", str(exe), str(ROOT / "tests/c/arena_smoke.c"), f"-I{ROOT / 'include'}",
                    f"-L{lib_dir}", "-lonitama_az", f"-Wl,-rpath,{lib_dir}", f"-L{rocm}", "-lamdhip64",
                    f"-Wl,-rpath,{rocm}", "-lm"], check=True)
    sims, max_plies, deal_seed, random_seed = 16, 60, 21, 500
    r = subprocess.run([str(exe), str(sims), str(max_plies), str(deal_seed), str(random_seed)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("fight ")]
    assert len(lines) == 2
    for i, w in enumerate(lines):  # the second fight ran on an engine created after the first was destroyed
        rc, st, results, plies = _hash_fight(lib, arena_config(EvaluatorConfig(game_amnt=6, max_plies=max_plies, seed=deal_seed)),
                                             sims, random_seed + i)
        assert rc == 0
        assert [int(x) for x in w[w.index("results") + 1: w.index("plies")]] == results
        assert [int(x) for x in w[w.index("plies") + 1: w.index("wld")]] == plies
        assert [int(x) for x in w[w.index("wld") + 1: w.index("passes")]] == [st.wins, st.loses, st.draws]
        assert float(w[w.index("ratings") + 1]) == st.rating_a and float(w[w.index("ratings") + 2]) == st.rating_b
    assert lines[0][4:] != lines[1][4:]  # (two Random seeds: two different fights)
