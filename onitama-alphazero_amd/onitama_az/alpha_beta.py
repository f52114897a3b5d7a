"""The reference's alpha-beta agent (onitama-game/src/ai/alpha_beta/mod.rs:15-183) on the GPU.

`AlphaBeta` mirrors the reference struct and Agent impl; every search runs in libonitama_az.so
(oaz_alphabeta_search: one GPU wave per root, one lane per root move). The reference deepens
iteratively up to max_depth - 1 plies and keeps only the last iteration's result, so a run its clock
does not cut equals one search to max_depth - 1 plies: that search runs here, and `search_time` is kept
for `id()` only and not enforced (as `Mcts.search_time`). `generate_moves_np` answers a batch of
positions at once (the arena's batched fights).

`alpha_beta_generate_move` (oaz_alphabeta_generate_move) is the agent with the reference's own settings:
max_depth up to 8 (bin/tournament.rs:107-110) and the search_time clock, as a split search that spreads one
root over thousands of lanes. `AlphaBeta(max_depth=7 | 8)` and `AlphaBeta(enforce_search_time=True)` go there.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _abi
from .game import DoneMove, GameState


def default_config() -> _abi.oaz_alphabeta_config:
    cfg = _abi.oaz_alphabeta_config()
    _abi.load().oaz_alphabeta_config_default(C.byref(cfg))
    return cfg


@dataclass
class AlphaBetaResult:
    moves: np.ndarray   # [G] MOVE_DTYPE (from == 25: pass, the root had no legal move)
    scores: np.ndarray  # [G] int32 best_score (Red maximises, Blue minimises; INT32_MIN / INT32_MAX untouched)
    stats: _abi.oaz_alphabeta_stats


def alpha_beta_evaluate(states: np.ndarray, move_results=None) -> np.ndarray:
    """Evaluation::evaluate (evaluation.rs:24-90) on the host: colour = to_move, move_results as MoveResult
    codes or None for Option::None."""
    states = np.ascontiguousarray(states, dtype=_abi.STATE_DTYPE).reshape(-1)
    mr = None if move_results is None else np.ascontiguousarray(move_results, dtype=np.uint8).reshape(-1)
    assert mr is None or len(mr) == len(states)
    out = np.zeros(len(states), dtype=np.int32)
    _abi.check(_abi.load().oaz_alphabeta_evaluate(_abi.ptr(states), None if mr is None else _abi.ptr(mr), len(states),
                                                  _abi.ptr(out)))
    return out


def alpha_beta_search(roots: np.ndarray, max_depth: int = 6, device: int = 0) -> AlphaBetaResult:
    """One search per root to max_depth - 1 plies (max_depth in 2..6)."""
    roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE).reshape(-1)
    cfg = default_config()
    cfg.max_depth, cfg.device = int(max_depth), int(device)
    G = len(roots)
    moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
    scores = np.zeros(G, dtype=np.int32)
    st = _abi.oaz_alphabeta_stats()
    _abi.check(_abi.load().oaz_alphabeta_search(_abi.ptr(roots), G, C.byref(cfg), _abi.ptr(moves), _abi.ptr(scores),
                                                C.byref(st)))
    return AlphaBetaResult(moves, scores, st)


@dataclass
class AlphaBetaAgentResult:
    moves: np.ndarray   # as AlphaBetaResult's
    scores: np.ndarray
    stats: _abi.oaz_alphabeta_agent_stats  # the last iteration's counts, its plies and split, the call's elapsed_ms


def alpha_beta_generate_move(roots: np.ndarray, max_depth: int = 6, search_time=None, split: int = 0,
                             device: int = 0) -> AlphaBetaAgentResult:
    """Agent::generate_move (mod.rs:136-170) for every root through oaz_alphabeta_generate_move: max_depth in
    2..8, the tree split over `split` levels (0: chosen from the batch and the depth). search_time in seconds is
    the reference's clock (iteration d starts while d < max_depth and the time is not up; the roots of the call
    share it); None or 0 runs the one search to max_depth - 1 plies."""
    roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE).reshape(-1)
    cfg = _abi.oaz_alphabeta_agent_config()
    _abi.load().oaz_alphabeta_agent_config_default(C.byref(cfg))
    cfg.max_depth, cfg.device, cfg.split = int(max_depth), int(device), int(split)
    cfg.search_time_ns = 0 if search_time is None else int(round(float(search_time) * 1e9))
    G = len(roots)
    moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
    scores = np.zeros(G, dtype=np.int32)
    st = _abi.oaz_alphabeta_agent_stats()
    _abi.check(_abi.load().oaz_alphabeta_generate_move(_abi.ptr(roots), G, C.byref(cfg), _abi.ptr(moves),
                                                       _abi.ptr(scores), C.byref(st)))
    return AlphaBetaAgentResult(moves, scores, st)


@dataclass
class AlphaBeta:  # ai/alpha_beta/mod.rs:15-28
    """With the defaults and max_depth <= 6 every search is oaz_alphabeta_search to max_depth - 1 plies and
    search_time is kept for id() only. max_depth 7 or 8, or enforce_search_time=True (the reference's clock,
    search_time seconds per call), go through the split search (alpha_beta_generate_move) with `split`."""
    max_depth: int = 6
    search_time: float = 1.0
    device: int = 0  # the GPU the searches run on (common.rs Options.device)
    enforce_search_time: bool = False
    split: int = 0   # the split search's levels (0: auto); unused on the default path

    def _deep(self) -> bool:
        return self.max_depth > 6 or self.enforce_search_time

    def _search(self, roots: np.ndarray):
        if self._deep():
            return alpha_beta_generate_move(roots, self.max_depth, self.search_time if self.enforce_search_time else None,
                                            self.split, self.device)
        return alpha_beta_search(roots, self.max_depth, self.device)

    def generate_move(self, game_state: GameState) -> Tuple[DoneMove, float]:  # mod.rs:136-170
        r = self._search(game_state.state.to_np(game_state.curr_player_color))
        return DoneMove.from_c(r.moves[0]), float(r.scores[0])

    def generate_moves_np(self, roots: np.ndarray) -> np.ndarray:
        return self._search(roots).moves

    def reserve(self, n: int) -> None:
        pass

    def device_key(self):  # a stateless GPU search (its own buffers and stream per call): may run beside an engine's
        return ("alpha_beta", id(self))

    def name(self) -> str:  # mod.rs:172-174
        return "AlphaBeta AI"

    def id(self) -> int:  # mod.rs:180-182
        return int(self.search_time * 1e9) + self.max_depth
