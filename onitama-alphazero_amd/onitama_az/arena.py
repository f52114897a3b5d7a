"""The arena's fight on the device: `native_fight` is `evaluator.fight` through oaz_arena_fight.

The game states stay on the GPU for the whole fight (routing, the Random agent and the move application are
kernels of oaz_arena.hip; an AlphaZero side's engine searches the roots where the router left them), the
host reads two counts per ply, and Elo is folded over the results in game order at the end, so the
statistics equal `evaluator.fight`'s game for game for the same agents and seeds. `native_fight(slots=S)` plays
the same fight on a pool of S game slots that are refilled on the device as games end (oaz_arena_fight_slots).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from .evaluator import AlphaZeroAgent, EvaluatorConfig, FightStatistics, RatingChange, WinLoseDraws
from .mcts import _search_engine


@dataclass
class NativeRandomAgent:
    """The reference's Random agent (ai/random.rs:11-43) as the arena's kernel: the draws of game k at ply p
    are Philox(seed; k, 0x52414E44, p) (oaz_random_agent_move), whatever the batch the game is moved in."""
    seed: int = 0

    def name(self) -> str:
        return "Random AI"

    # In `evaluator.fight` (the host loop) the same draws come from the host-only oaz_random_agent_move: fight
    # names the games and their plies of the coming batch through begin_turn.
    def reserve(self, n: int) -> None:
        pass

    def begin_turn(self, games, plies) -> None:
        self._turn = (np.asarray(games, dtype=np.uint64), np.asarray(plies, dtype=np.uint32))

    def generate_moves_np(self, roots: np.ndarray) -> np.ndarray:
        roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE).reshape(-1)
        games, plies = self._turn
        assert len(games) == len(roots), "begin_turn names the games of this batch"
        out = np.zeros(len(roots), dtype=_abi.MOVE_DTYPE)
        lib = _abi.load()
        for i in range(len(roots)):
            _abi.check(lib.oaz_random_agent_move(int(self.seed), int(games[i]), int(plies[i]), _abi.ptr(roots[i:i + 1]),
                                                 _abi.ptr(out[i:i + 1])))
        return out


def arena_config(config: EvaluatorConfig, device: int = 0) -> _abi.oaz_arena_config:
    c = _abi.oaz_arena_config()
    _abi.load().oaz_arena_config_default(C.byref(c))
    c.game_amnt, c.max_plies, c.device, c.seed = int(config.game_amnt), int(config.max_plies), int(device), int(config.seed)
    if config.deck is not None:
        c.fixed_deck = 1
        for i, card in enumerate(config.deck.indices()):
            c.deck[i] = int(card)
    return c


def arena_capacity(cfg: _abi.oaz_arena_config):
    """Largest batch (agent, opponent) answer per ply in a fight of cfg (oaz_arena_capacity)."""
    out = (C.c_int32 * 2)()
    _abi.check(_abi.load().oaz_arena_capacity(C.byref(cfg), C.byref(out)))
    return int(out[0]), int(out[1])


def arena_slots_capacity(cfg: _abi.oaz_arena_config, slots: int):
    """Largest batch (agent, opponent) answer per round in a fight of cfg on `slots` slots
    (oaz_arena_slots_capacity): arena_capacity's for slots >= game_amnt, else (slots, slots)."""
    out = (C.c_int32 * 2)()
    _abi.check(_abi.load().oaz_arena_slots_capacity(C.byref(cfg), int(slots), C.byref(out)))
    return int(out[0]), int(out[1])


def _device_of(agent) -> int:
    if isinstance(agent, AlphaZeroAgent):
        return int(agent.mcts.model.options.device)
    return int(getattr(agent, "device", -1))


def _describe(agent, need: int) -> _abi.oaz_arena_agent:
    from .alpha_beta import AlphaBeta
    from .pure_mcts import Mcts, default_config
    a = _abi.oaz_arena_agent()
    if isinstance(agent, AlphaZeroAgent):
        agent.reserve(need)
        eng = _search_engine(agent.mcts._cache, agent.mcts.config, agent.mcts.model, agent.capacity)
        a.kind, a.engine = _abi.AGENT_ALPHAZERO, eng.handle
    elif isinstance(agent, NativeRandomAgent):
        a.kind, a.seed = _abi.AGENT_RANDOM, int(agent.seed)
    elif isinstance(agent, Mcts):
        m = default_config()
        m.max_playouts, m.min_node_visits = int(agent.max_playouts), int(agent.min_node_visits)
        m.exploration_c, m.seed, m.rollout_cap = float(agent.exploration_c), int(agent.seed), 1000  # (pure_mcts_search's)
        a.kind, a.mcts = _abi.AGENT_PURE_MCTS, m
    elif isinstance(agent, AlphaBeta):
        a.kind = _abi.AGENT_ALPHABETA
        a.alphabeta.max_depth = int(agent.max_depth)
    else:
        raise TypeError(f"native_fight: {type(agent).__name__} has no native form "
                        "(AlphaZeroAgent, NativeRandomAgent, Mcts, AlphaBeta)")
    return a


def native_fight(config: EvaluatorConfig, agent, opponent, agent_rating: float = 800.0,
                 opponent_rating: float = 800.0, slots=None) -> FightStatistics:
    """evaluator.rs:355-399 as one oaz_arena_fight call. The agents are the objects `evaluator.fight` takes
    (AlphaZeroAgent, Mcts, AlphaBeta) or a NativeRandomAgent; an AlphaZeroAgent's shared search engine is
    sized for the batch the fight needs and searched with the agent's config. A pure-MCTS side's c-th search of
    the fight draws from the streams `evaluator.fight` gives a fresh Mcts object's c-th call (c << 20). The
    returned statistics also carry `passes` and `plies_total` (oaz_fight_stats).

    slots=S plays the fight on min(S, game_amnt) game slots through oaz_arena_fight_slots (`evaluator.fight_slots`
    is its host-loop statement): a finished slot is dealt the fight's next game on the device, the engines are
    sized for S slots instead of game_amnt games, and the statistics equal the lock-step fight's game for game
    for every agent but a pure-MCTS one, whose streams follow the slots (include/onitama_az.h). They then also
    carry `rounds`, `searches`, `max_batch` and `slots` (oaz_arena_slots_stats). slots=None is the lock-step call."""
    devs = {d for d in (_device_of(agent), _device_of(opponent)) if d >= 0}
    if len(devs) > 1:
        raise ValueError(f"native_fight: the agents are on different devices {sorted(devs)}")
    cfg = arena_config(config, devs.pop() if devs else 0)
    need = arena_capacity(cfg) if slots is None else arena_slots_capacity(cfg, slots)
    # (an engine shared by both sides is made once, for the larger need: both needs are equal)
    sides = [_describe(agent, need[0]), _describe(opponent, need[1])]
    if sides[0].kind == sides[1].kind == _abi.AGENT_ALPHAZERO and agent.mcts.model is opponent.mcts.model:
        sides[0] = _describe(agent, need[0])  # the opponent's reserve may have rebuilt the shared engine
        if (agent.mcts.config.max_playouts, agent.mcts.config.exploration_c, agent.mcts.config.train) != (
                opponent.mcts.config.max_playouts, opponent.mcts.config.exploration_c, opponent.mcts.config.train):
            raise ValueError("native_fight: two agents on one engine need the same search config")
    n = cfg.game_amnt
    st = _abi.oaz_fight_stats()
    results = np.zeros(n, dtype=np.uint8)
    plies = np.zeros(n, dtype=np.int32)
    history = np.zeros((n, 4), dtype=np.float64)
    if slots is None:
        _abi.check(_abi.load().oaz_arena_fight(C.byref(cfg), C.byref(sides[0]), C.byref(sides[1]), float(agent_rating),
                                               float(opponent_rating), C.byref(st), _abi.ptr(results), _abi.ptr(plies),
                                               _abi.ptr(history)))
    else:
        ss = _abi.oaz_arena_slots_stats()
        _abi.check(_abi.load().oaz_arena_fight_slots(C.byref(cfg), int(slots), C.byref(sides[0]), C.byref(sides[1]),
                                                     float(agent_rating), float(opponent_rating), C.byref(st),
                                                     _abi.ptr(results), _abi.ptr(plies), _abi.ptr(history), C.byref(ss)))
    out = FightStatistics(st.rating_a, st.rating_b)
    out.general = WinLoseDraws(st.wins, st.loses, st.draws)
    out.color = [WinLoseDraws(st.color_wins[c], st.color_loses[c], st.color_draws[c]) for c in (0, 1)]
    out.winrate, out.color_winrate = float(st.winrate), [float(st.color_winrate[0]), float(st.color_winrate[1])]
    out.rating_change_history = [RatingChange(*map(float, h)) for h in history]
    out.results = [int(r) for r in results]
    out.plies = [int(p) for p in plies]
    out.passes = int(st.passes)
    out.plies_total = int(st.plies_total)
    if slots is not None:
        out.rounds, out.slots = int(ss.rounds), int(ss.slots)
        out.searches, out.max_batch = [int(x) for x in ss.searches], [int(x) for x in ss.max_batch]
    return out
