"""The host side of the arena's pool of refilled game slots (include/onitama_az.h, oaz_arena_fight_slots): the
statistics struct, oaz_arena_slots_capacity and the argument checks, none of which touches a device."""
import ctypes as C

import numpy as np

from onitama_az import _abi


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


def _fight(lib, cfg, a, b, slots=None):
    """(rc, message) of oaz_arena_fight (slots None) or oaz_arena_fight_slots."""
    st = _abi.oaz_fight_stats()
    if slots is None:
        rc = lib.oaz_arena_fight(C.byref(cfg), C.byref(a), C.byref(b), 800.0, 800.0, C.byref(st), None, None, None)
    else:
        rc = lib.oaz_arena_fight_slots(C.byref(cfg), slots, C.byref(a), C.byref(b), 800.0, 800.0, C.byref(st), None, None,
                                       None, None)
    return rc, lib.oaz_last_error().decode()


def test_slots_stats_layout():
    assert C.sizeof(_abi.oaz_arena_slots_stats) == 40
    f = _abi.oaz_arena_slots_stats
    assert (f.rounds.offset, f.searches.offset, f.max_batch.offset, f.slots.offset, f.reserved.offset) == (0, 8, 24, 32, 36)


def test_slots_capacity(lib):
    out, ref = (C.c_int32 * 2)(), (C.c_int32 * 2)()
    for cfg in (_cfg(lib, game_amnt=33, seed=5), _cfg(lib, game_amnt=7, deck=[0, 1, 2, 3, 4])):
        n = cfg.game_amnt
        assert lib.oaz_arena_capacity(C.byref(cfg), C.byref(ref)) == 0
        for slots in (n, n + 1, 4 * n):  # nothing is refilled: the lock-step fight's batches
            assert lib.oaz_arena_slots_capacity(C.byref(cfg), slots, C.byref(out)) == 0
            assert tuple(out) == tuple(ref)
        for slots in (1, 2, n - 1):  # slots at different plies can all be one side's turn
            assert lib.oaz_arena_slots_capacity(C.byref(cfg), slots, C.byref(out)) == 0
            assert tuple(out) == (slots, slots)
    assert tuple(ref) == (4, 4) and 7 - 1 > 4  # (below game_amnt the pool asks for more than the lock-step fight)
    assert lib.oaz_arena_slots_capacity(C.byref(_cfg(lib, game_amnt=0)), 3, C.byref(out)) == 0 and tuple(out) == (0, 0)
    for slots in (0, -1):
        assert lib.oaz_arena_slots_capacity(C.byref(_cfg(lib)), slots, C.byref(out)) == _abi.ERR_ARG
        assert lib.oaz_last_error()
    assert lib.oaz_arena_slots_capacity(None, 3, C.byref(out)) == _abi.ERR_ARG
    assert lib.oaz_arena_slots_capacity(C.byref(_cfg(lib)), 3, None) == _abi.ERR_ARG


def test_python_slots_capacity(lib):
    from onitama_az.arena import arena_capacity, arena_config, arena_slots_capacity
    from onitama_az.evaluator import EvaluatorConfig
    cfg = arena_config(EvaluatorConfig(game_amnt=33, seed=5))
    assert arena_slots_capacity(cfg, 33) == arena_capacity(cfg) and arena_slots_capacity(cfg, 4) == (4, 4)


def test_bad_slot_counts(lib):
    rnd = _agent(_abi.AGENT_RANDOM)
    for slots in (0, -1):
        rc, msg = _fight(lib, _cfg(lib), rnd, rnd, slots)
        assert rc == _abi.ERR_ARG and "slots" in msg
        rc, msg = _fight(lib, _cfg(lib, game_amnt=0), rnd, rnd, slots)  # (also with nothing to play)
        assert rc == _abi.ERR_ARG and "slots" in msg


def test_zero_games_is_ok_without_a_device(lib):
    for a, b in ((_agent(_abi.AGENT_RANDOM), _agent(_abi.AGENT_ALPHABETA)),
                 (_agent(_abi.AGENT_PURE_MCTS), _agent(_abi.AGENT_RANDOM))):
        st, ss = _abi.oaz_fight_stats(), _abi.oaz_arena_slots_stats()
        st.wins, ss.rounds, ss.slots, ss.max_batch[1] = 9, 7, 3, 5
        rc = lib.oaz_arena_fight_slots(C.byref(_cfg(lib, game_amnt=0)), 4, C.byref(a), C.byref(b), 812.5, 790.0,
                                       C.byref(st), None, None, None, C.byref(ss))
        assert rc == 0
        assert (st.rating_a, st.rating_b, st.wins, st.loses, st.draws, st.plies_total, st.passes) == (812.5, 790.0, 0, 0,
                                                                                                      0, 0, 0)
        assert st.winrate == 0.0 and list(st.color_winrate) == [0.0, 0.0]
        assert (ss.rounds, list(ss.searches), list(ss.max_batch), ss.slots, ss.reserved) == (0, [0, 0], [0, 0], 0, 0)


def test_argument_errors_equal_the_lock_step_entry(lib, orc):
    rnd = _agent(_abi.AGENT_RANDOM)
    good = orc.initial_state([0, 1, 2, 3, 4])
    bad = good.copy()
    bad["cards"][0][2] = 16
    starts = np.concatenate([good, bad])
    with_start = _cfg(lib, game_amnt=2)
    with_start.start = starts.ctypes.data
    cases = [
        (_cfg(lib), _agent(7), rnd),                                       # unknown kind
        (_cfg(lib), rnd, _agent(-1)),
        (_cfg(lib), _agent(_abi.AGENT_ALPHAZERO), rnd),                    # no engine
        (_cfg(lib), rnd, _agent(_abi.AGENT_ALPHAZERO)),
        (_cfg(lib, deck=[0, 1, 2, 3, 16]), rnd, rnd),                      # card >= 16
        (_cfg(lib, deck=[0, 1, 2, 1, 4]), rnd, rnd),                       # repeated card
        (with_start, rnd, rnd),                                            # a start position that is no state
        (_cfg(lib), _agent(_abi.AGENT_ALPHABETA, max_depth=7), rnd),       # max_depth outside 2..6
        (_cfg(lib), rnd, _agent(_abi.AGENT_ALPHABETA, max_depth=1)),
        (_cfg(lib, game_amnt=-1), rnd, rnd),
        (_cfg(lib, game_amnt=0, deck=[5, 5, 1, 2, 3]), rnd, rnd),          # checked with nothing to play too
    ]
    for cfg, a, b in cases:
        ref = _fight(lib, cfg, a, b)
        assert ref[0] == _abi.ERR_ARG and ref[1]
        for slots in (1, 3, 1000):
            assert _fight(lib, cfg, a, b, slots) == ref
    st = _abi.oaz_fight_stats()
    assert lib.oaz_arena_fight_slots(None, 2, C.byref(rnd), C.byref(rnd), 800.0, 800.0, C.byref(st), None, None, None,
                                     None) == _abi.ERR_ARG
    assert lib.oaz_arena_fight_slots(C.byref(_cfg(lib)), 2, None, C.byref(rnd), 800.0, 800.0, C.byref(st), None, None,
                                     None, None) == _abi.ERR_ARG
    assert lib.oaz_arena_fight_slots(C.byref(_cfg(lib)), 2, C.byref(rnd), C.byref(rnd), 800.0, 800.0, None, None, None,
                                     None, None) == _abi.ERR_ARG
