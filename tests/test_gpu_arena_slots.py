"""A fight on a pool of refilled game slots (oaz_arena_fight_slots, arena.native_fight(slots=S)). For every agent
whose answer depends only on the position or on (game, ply) the results equal the lock-step fight's game for
game, so the references are the ones the lock-step fight is tested against: the sequential host loop for the
HASH evaluator against Random (tests/arena_util.py) and the lock-step native fight. A pure-MCTS side's streams
follow the slots: its reference is the host-loop statement of the schedule, `evaluator.fight_slots`."""
import ctypes as C

import numpy as np
import pytest

from arena_util import C_PUCT, sequential_hash_vs_random
from onitama_az import _abi
from onitama_az.alpha_beta import AlphaBeta
from onitama_az.arena import NativeRandomAgent, arena_config, arena_slots_capacity, native_fight
from onitama_az.engine import Engine
from onitama_az.evaluator import AlphaZeroAgent, Evaluator, EvaluatorConfig, fight_slots
from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNet, ConvResNetConfig
from onitama_az.pure_mcts import Mcts

pytestmark = pytest.mark.gpu


def simulate(plies, slots):
    """The schedule on the host from the games' lengths alone: (rounds, moves made)."""
    n, s = len(plies), min(slots, len(plies))
    left, nxt, rounds = list(plies[:s]), s, 0  # plies a slot's game still has; -1: the slot is empty
    while True:
        for i in range(s):  # harvest and refill, ascending slot order
            if left[i] == 0:
                left[i], nxt = (plies[nxt], nxt + 1) if nxt < n else (-1, nxt)
        if all(x < 0 for x in left):
            return rounds, sum(plies)
        rounds += 1
        left = [x - 1 if x > 0 else x for x in left]  # every active slot moves exactly once


def test_simulator_on_the_recorded_lengths():
    a = [11, 20, 13, 17, 11, 10, 5, 9, 12, 22, 5, 17]
    assert [simulate(a, s)[0] for s in (1, 2, 3, 5, 7, 12, 13)] == [152, 79, 58, 39, 33, 22, 22]
    b = [11, 14, 11, 9, 46, 11, 9, 20, 16, 62, 11, 11]
    assert [simulate(b, s)[0] for s in (1, 2, 3, 5, 7, 12)] == [231, 130, 107, 82, 73, 62]


def _net(seed):
    return ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=seed)


@pytest.fixture(scope="module")
def nets():
    return _net(11), _net(12)


def _mcfg(sims):
    return AlphaZeroMctsConfig(exploration_c=C_PUCT, max_playouts=sims, train=False, enforce_search_time=False)


def _az(nets, sims):
    return AlphaZeroAgent(_mcfg(sims), nets[0]), AlphaZeroAgent(_mcfg(sims), nets[1])


def _assert_same(nat, ref):  # (tests/test_gpu_arena.py's)
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


def _assert_schedule(nat, slots, cap):
    """The statistics of a slots fight against the simulator run on its own game lengths."""
    rounds, moves = simulate(nat.plies, slots)
    assert (nat.rounds, nat.plies_total, nat.slots) == (rounds, moves, min(slots, len(nat.plies)))
    assert all(b <= c for b, c in zip(nat.max_batch, cap)) and all(s <= rounds for s in nat.searches)
    assert nat.searches[0] + nat.searches[1] >= rounds


# ---- HASH evaluator vs Random: the C entry point against the sequential host loop ---------------------------
def _hash_fight(lib, cfg, slots, sims, random_seed, games=None):
    need = arena_slots_capacity(cfg, slots)
    with Engine(games=max(games if games is not None else need[0], 1), sims=sims, c_puct=C_PUCT, train_noise=0,
                evaluator=_abi.EVAL_HASH, blocks=0) as eng:
        a, b = _abi.oaz_arena_agent(), _abi.oaz_arena_agent()
        a.kind, a.engine = _abi.AGENT_ALPHAZERO, eng.handle
        b.kind, b.seed = _abi.AGENT_RANDOM, random_seed
        n = cfg.game_amnt
        st, ss = _abi.oaz_fight_stats(), _abi.oaz_arena_slots_stats()
        results, plies, hist = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, 4))
        rc = lib.oaz_arena_fight_slots(C.byref(cfg), slots, C.byref(a), C.byref(b), 800.0, 800.0, C.byref(st),
                                       _abi.ptr(results), _abi.ptr(plies), _abi.ptr(hist), C.byref(ss))
        return rc, st, ss, [int(r) for r in results], [int(p) for p in plies], need


@pytest.fixture(scope="module")
def sequential(lib, orc):
    """The sequential loop's 12 games (deal seed 5, Random seed 77, max_plies 60) per simulation count."""
    return {sims: sequential_hash_vs_random(orc, lib, 12, 60, 5, 77, sims) for sims in (16, 4)}


@pytest.mark.parametrize("sims,slots,rounds", [(16, s, r) for s, r in zip((1, 2, 3, 5, 7, 12, 13), (152, 79, 58, 39, 33, 22, 22))] +
                         [(4, s, r) for s, r in zip((1, 2, 3, 5, 7, 12), (231, 130, 107, 82, 73, 62))])
def test_hash_vs_random_equals_sequential_host_loop(lib, sequential, sims, slots, rounds):
    """slots 1 is the fully sequential fight, slots >= 12 the lock-step one. With 4 simulations game 9 is cut by
    the ply budget inside a refilled pool. `rounds` are the values worked out on the host for the lengths
    [11, 20, 13, 17, 11, 10, 5, 9, 12, 22, 5, 17] (16 sims) and [11, 14, 11, 9, 46, 11, 9, 20, 16, 62, 11, 11] (4)."""
    ref_results, ref_plies, ref_passes, _ = sequential[sims]
    assert len(set(ref_plies)) > 1  # (the slots do get out of step)
    if sims == 4:
        # a game cut by the budget: 62 plies at max_plies 60 and no win (its last move took nothing: IN_PROGRESS)
        assert (ref_plies[9], ref_results[9]) == (62, _abi.IN_PROGRESS)
    rc, st, ss, results, plies, need = _hash_fight(lib, arena_config(EvaluatorConfig(game_amnt=12, max_plies=60, seed=5)),
                                                   slots, sims, 77)
    assert rc == 0, lib.oaz_last_error()
    assert (results, plies, st.passes) == (ref_results, ref_plies, ref_passes)
    assert (ss.rounds, st.plies_total) == simulate(ref_plies, slots) and ss.rounds == rounds
    assert ss.slots == min(slots, 12) and ss.reserved == 0
    assert all(0 < ss.max_batch[s] <= need[s] for s in (0, 1))
    assert all(0 < ss.searches[s] <= ss.rounds for s in (0, 1)) and ss.searches[0] + ss.searches[1] >= ss.rounds
    if slots == 1:
        assert ss.searches[0] + ss.searches[1] == ss.rounds and list(ss.max_batch) == [1, 1]


def test_passes_from_start_positions(lib, orc):
    """The stuck position of test_gpu_arena.py's test_passes_equal_sequential_host_loop in four games on three slots."""
    bit = lambda sq: 0x80000000 >> sq  # noqa: E731
    stuck = orc.state([bit(0), bit(24)], [bit(5) | bit(10) | bit(15) | bit(20), bit(9) | bit(19)], [0, 11, 2, 3, 5], 0)
    assert len(orc.movegen(stuck[0])) == 0
    starts = np.concatenate([stuck] * 4)
    ref_results, ref_plies, ref_passes, _ = sequential_hash_vs_random(orc, lib, 4, 60, 0, 13, 16, starts=starts)
    assert ref_passes >= 2
    cfg = arena_config(EvaluatorConfig(game_amnt=4, max_plies=60))
    cfg.start = starts.ctypes.data
    rc, st, ss, results, plies, _ = _hash_fight(lib, cfg, 3, 16, 13)
    assert rc == 0, lib.oaz_last_error()
    assert (results, plies, st.passes) == (ref_results, ref_plies, ref_passes)
    assert (ss.rounds, st.plies_total) == simulate(ref_plies, 3)


def test_engine_smaller_than_the_pool(lib):
    cfg = arena_config(EvaluatorConfig(game_amnt=12, max_plies=60, seed=5))
    rc = _hash_fight(lib, cfg, 5, 4, 1, games=4)[0]
    assert rc == _abi.ERR_CAPACITY and lib.oaz_last_error()


# ---- network vs network: against the lock-step native fight ------------------------------------------------------
@pytest.fixture(scope="module")
def lock_step_33(nets):
    return native_fight(EvaluatorConfig(game_amnt=33, max_plies=40, seed=5), *_az(nets, 24), 812.0, 790.0)


@pytest.mark.parametrize("slots", [1, 3, 7, 32, 33, 64])
def test_alphazero_fight_equals_lock_step(nets, lock_step_33, slots):
    """(Also pins the small-batch network kernel to the large-batch one bit for bit, across batch sizes.)"""
    cfg = EvaluatorConfig(game_amnt=33, max_plies=40, seed=5)
    nat = native_fight(cfg, *_az(nets, 24), 812.0, 790.0, slots=slots)
    _assert_same(nat, lock_step_33)
    _assert_schedule(nat, slots, arena_slots_capacity(arena_config(cfg), slots))
    if slots >= 33:
        assert nat.rounds == max(lock_step_33.plies)


def test_one_engine_on_both_sides(nets):
    cfg = EvaluatorConfig(game_amnt=9, max_plies=40, seed=6)
    one = lambda: (AlphaZeroAgent(_mcfg(24), nets[0]), AlphaZeroAgent(_mcfg(24), nets[0]))  # noqa: E731
    nat = native_fight(cfg, *one(), slots=4)
    _assert_same(nat, native_fight(cfg, *one()))
    _assert_schedule(nat, 4, (4, 4))


@pytest.fixture(scope="module")
def lock_step_3000(nets):
    return native_fight(EvaluatorConfig(game_amnt=3000, max_plies=150, seed=7), *_az(nets, 2))


@pytest.mark.parametrize("slots", [1025, 2049])
def test_pool_past_one_scan_block(nets, lock_step_3000, slots):
    """More slots than the refill's 1 024 threads, odd counts (two and three slots per thread), and many slots
    refilled in one round."""
    assert len(set(lock_step_3000.plies)) > 8
    nat = native_fight(EvaluatorConfig(game_amnt=3000, max_plies=150, seed=7), *_az(nets, 2), slots=slots)
    _assert_same(nat, lock_step_3000)
    _assert_schedule(nat, slots, (slots, slots))


@pytest.mark.parametrize("max_plies,cut_len", [(150, 152), (0, 2), (-1, 1)])
def test_ply_budget(nets, max_plies, cut_len):
    cfg = EvaluatorConfig(game_amnt=6, max_plies=max_plies, seed=8)
    nat = native_fight(cfg, *_az(nets, 2), slots=2)
    _assert_same(nat, native_fight(cfg, *_az(nets, 2)))
    _assert_schedule(nat, 2, (2, 2))
    for r, n in zip(nat.results, nat.plies):
        assert n <= cut_len and ((r in (1, 2)) or n == cut_len)  # evaluator.rs:376-389
    if max_plies <= 0:  # both slots finish in the same round every time
        assert nat.plies == [cut_len] * 6 and nat.rounds == 3 * cut_len


# ---- the other opponents ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [4, 3])
def test_alphabeta_opponent_equals_lock_step(nets, max_depth):
    cfg = EvaluatorConfig(game_amnt=8, max_plies=60, seed=10)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), AlphaBeta(max_depth=max_depth), slots=3)
    _assert_same(nat, native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), AlphaBeta(max_depth=max_depth)))
    _assert_schedule(nat, 3, (3, 3))


@pytest.mark.parametrize("mcts_is_agent", [False, True])
def test_pure_mcts_side_equals_host_loop_statement(nets, mcts_is_agent):
    """The stream rule with slots for games: the side's c-th search draws from c << 20 on, root g being its g-th
    root in ascending slot order. `fight_slots` gives a fresh Mcts object's c-th call the same streams."""
    cfg = EvaluatorConfig(game_amnt=8, max_plies=60, seed=9)
    mk = lambda: Mcts(search_time=0.4, min_node_visits=5, exploration_c=1.41, max_playouts=50, seed=31)  # noqa: E731
    if mcts_is_agent:
        pair = lambda: (mk(), AlphaZeroAgent(_mcfg(16), nets[1]))  # noqa: E731
    else:
        pair = lambda: (AlphaZeroAgent(_mcfg(16), nets[0]), mk())  # noqa: E731
    nat = native_fight(cfg, *pair(), slots=3)
    ref = fight_slots(cfg, *pair(), slots=3)
    _assert_same(nat, ref)
    assert nat.rounds == ref.rounds
    _assert_schedule(nat, 3, (3, 3))
    _assert_same(native_fight(cfg, *pair(), slots=3), nat)     # deterministic
    _assert_same(native_fight(cfg, *pair(), slots=8), native_fight(cfg, *pair()))  # nothing refilled: the lock-step streams


def test_fight_slots_equals_native_for_random(nets):
    """begin_turn names the slots' games and plies: NativeRandomAgent's draws are keyed by them."""
    cfg = EvaluatorConfig(game_amnt=12, max_plies=60, seed=5)
    nat = native_fight(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), NativeRandomAgent(77), slots=5)
    ref = fight_slots(cfg, AlphaZeroAgent(_mcfg(16), nets[0]), NativeRandomAgent(77), slots=5)
    _assert_same(nat, ref)
    assert nat.rounds == ref.rounds
    assert len(set(nat.plies)) > 1
    _assert_schedule(nat, 5, (5, 5))


# ---- pit ---------------------------------------------------------------------------------------------------------
def test_pit_native_slots():
    best, new = _net(21), _net(22)
    config = EvaluatorConfig(game_amnt=4, max_plies=60, seed=9)
    ratings = ((800.0, 800.0), (820.0, 700.0), (800.0, 900.0), (810.0, 805.0))
    ev = Evaluator(config, best, new, ratings)
    pool, _ = ev.pit(sims=16, alphabeta=True, enforce_search_time=False, native=True, slots=2)
    ref, _ = ev.pit(sims=16, alphabeta=True, enforce_search_time=False, native=True)
    for a, b in ((pool.self_fight, ref.self_fight), (pool.random_fight, ref.random_fight),
                 (pool.alphabeta_fight, ref.alphabeta_fight)):
        _assert_same(a, b)
        assert a.slots == 2
    mcfg = AlphaZeroMctsConfig(search_time=0.4, max_playouts=16, train=False, enforce_search_time=False)
    mcts = Mcts(search_time=0.4, min_node_visits=5, exploration_c=1.41, max_playouts=16, seed=config.seed)
    _assert_same(pool.mcts_fight, fight_slots(config, AlphaZeroAgent(mcfg, _net(22)), mcts, *ratings[2], slots=2))
    with pytest.raises(ValueError):
        ev.pit(sims=16, slots=2)
