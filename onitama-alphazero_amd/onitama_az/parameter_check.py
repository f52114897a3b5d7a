"""The pure-MCTS parameter sweep: alphazero-training/src/bin/mcts_parameter_check.rs.

`ParameterCheck("c", C_VALUES).play()` plays `Mcts` against `Mcts` for every pair of values of `exploration_c`
(`"n"`: of `min_node_visits`), `game_amnt` games per pairing, the first-named value playing Red in even games
(`agent_color.switch()` and `agents.swap`, :36-43). The reference starts a thread per pairing; here all pairings'
games advance in lock step and every ply is one `pure_mcts_search_each` launch, each root carrying its mover's
parameters. Game q = p * game_amnt + j is game j of pairing p: it is dealt oaz_deal_deck(seed, q), and its search
at ply t draws from rollout stream (t << 20) + q, so an answer depends only on the position, the mover's
parameters, the seed and (t, q), and `play(sequential=True)` (pairing after pairing, one launch per pairing and
ply) plays the same games move for move.

Defined where the reference is not (as tournament.py): a game cut by the ply budget (:26-30, `game -= 1`
underflows at game 0) is a no-result: it is counted in `cut`, it is no win, it stays in the winrate's
denominator (the reference divides by game_amnt) and it is not replayed.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _abi
from .evaluator import _apply
from .game import Deck, initial_state_np
from .pure_mcts import pure_mcts_search_each

C_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0)  # mcts_parameter_check.rs:51
N_VALUES = tuple(range(9))                       # :91
MAX_GAMES = 1 << 20   # a stream is (ply << 20) + game
MAX_PLIES = 1 << 12   # and stays below 2^32


def pairings(values: Sequence) -> List[Tuple[int, int]]:
    """(i, k) for every i, then every k > i (:53-62, :93-102)."""
    return [(i, k) for i in range(len(values)) for k in range(i + 1, len(values))]


def format_line(kind: str, first, second, winrate: float) -> str:
    """The reference's result line (:78-83, :118-123)."""
    if kind == "c":
        return f"MCTS with c = {first:3.2f} vs MCTS with c = {second:3.2f} -> winrate: {winrate:3.2f}"
    return f"MCTS with n = {first} vs MCTS with n = {second} -> winrate: {winrate:3.2f}"


def fold_results(results: Sequence[int]) -> Tuple[int, int]:
    """(wins of the first-named value, games without a winner) of a pairing's last MoveResult codes in game
    order: the first-named value plays Red in even games (:36-43)."""
    wins = cut = 0
    for j, r in enumerate(results):
        if r not in (_abi.RED_WIN, _abi.BLUE_WIN):
            cut += 1
        elif r == (_abi.RED_WIN if j % 2 == 0 else _abi.BLUE_WIN):
            wins += 1
    return wins, cut


@dataclass
class PairingResult:
    first: float                # the two values, the first-named playing Red in even games
    second: float
    wins: int                   # of the first-named
    cut: int                    # games ended by the ply budget: no result
    winrate: float              # wins / game_amnt
    results: List[int]          # every game's last MoveResult
    plies: List[int]


class ParameterCheck:
    def __init__(self, kind: str, values: Sequence, game_amnt: int = 100, max_playouts: int = 1600,
                 search_time: float = 0.4, enforce_search_time: bool = False, min_node_visits: int = 1,
                 exploration_c: float = 1.0, max_plies: int = 150, seed: int = 20260101, device: int = 0,
                 verbose: bool = True):
        if kind not in ("c", "n"):
            raise ValueError(f"ParameterCheck: kind {kind!r} (\"c\" or \"n\")")
        self.kind, self.values = kind, tuple(values)
        self.game_amnt, self.max_playouts, self.max_plies = int(game_amnt), int(max_playouts), int(max_plies)
        self.search_time, self.enforce_search_time = float(search_time), bool(enforce_search_time)
        self.min_node_visits, self.exploration_c = int(min_node_visits), float(exploration_c)  # the one not swept
        self.seed, self.device, self.verbose = int(seed), int(device), verbose
        self.pairings = pairings(self.values)
        if self.game_amnt * len(self.pairings) > MAX_GAMES:
            raise ValueError(f"ParameterCheck: {self.game_amnt} games x {len(self.pairings)} pairings exceed 2^20")
        if self.max_plies + 2 > MAX_PLIES:
            raise ValueError(f"ParameterCheck: max_plies {self.max_plies}")
        self.launches = self.searches = 0  # of the last play()

    def _play_games(self, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Games q (ascending) in lock step, one launch per ply: (last MoveResult, plies) per game."""
        n = len(q)
        states = np.concatenate([initial_state_np(Deck.default(self.seed, int(k)).indices()) for k in q])
        p, j = q // self.game_amnt, q % self.game_amnt
        first = np.array([self.values[self.pairings[k][0]] for k in p])
        second = np.array([self.values[self.pairings[k][1]] for k in p])
        by_colour = np.where((j % 2 == 0)[None, :], np.stack([first, second]), np.stack([second, first]))  # [Red, Blue]
        progress = np.full(n, _abi.IN_PROGRESS, dtype=np.uint8)
        active = np.ones(n, dtype=bool)
        budget = np.full(n, self.max_plies, dtype=np.int64)
        plies = np.zeros(n, dtype=np.int64)
        t = 0
        while active.any():
            idx = np.where(active)[0]
            roots = np.ascontiguousarray(states[idx])
            mine = by_colour[roots["to_move"].astype(np.int64), idx]  # the mover's value
            r = pure_mcts_search_each(
                roots, self.max_playouts, mine.astype(np.int32) if self.kind == "n" else self.min_node_visits,
                mine.astype(np.float32) if self.kind == "c" else self.exploration_c,
                (t << 20) + q[idx].astype(np.uint64), self.seed,
                search_time=self.search_time if self.enforce_search_time else None, device=self.device)
            self.launches += 1
            self.searches += len(idx)
            progress[idx] = _apply(states, idx, r.moves)
            plies[idx] += 1
            won = (progress == _abi.RED_WIN) | (progress == _abi.BLUE_WIN)
            cut = active & ~won & (budget < 0)  # :26-32: tested after the move, then decremented
            budget[active] -= 1
            active &= ~won & ~cut
            t += 1
        return progress, plies

    def play(self, sequential: bool = False) -> List[PairingResult]:
        """Every pairing's games: all of them in lock step (one launch per ply), or with sequential=True pairing
        after pairing (one launch per pairing and ply). Both play the same games."""
        t0 = time.perf_counter()
        self.launches = self.searches = 0
        A, P = self.game_amnt, len(self.pairings)

        def fold(k: int, progress: np.ndarray, plies: np.ndarray) -> PairingResult:
            a, b = self.pairings[k]
            res = [int(x) for x in progress]
            wins, cut = fold_results(res)
            winrate = wins / A if A else float("nan")
            if self.verbose:
                print(format_line(self.kind, self.values[a], self.values[b], winrate), flush=True)
            return PairingResult(self.values[a], self.values[b], wins, cut, winrate, res, [int(x) for x in plies])

        if not A:
            out = [fold(k, np.zeros(0, np.uint8), np.zeros(0, np.int64)) for k in range(P)]
        elif sequential:  # every pairing's line as it ends
            out = [fold(k, *self._play_games(np.arange(k * A, (k + 1) * A, dtype=np.int64))) for k in range(P)]
        else:
            progress, plies = self._play_games(np.arange(A * P, dtype=np.int64)) if P else (None, None)
            out = [fold(k, progress[k * A:(k + 1) * A], plies[k * A:(k + 1) * A]) for k in range(P)]
        if self.verbose:
            print(f"Elapsed: {time.perf_counter() - t0:.3f}s\n", flush=True)
        return out


def play_with_c_value(**kw) -> List[PairingResult]:  # :49-87
    return ParameterCheck("c", C_VALUES, **kw).play()


def play_with_n_value(**kw) -> List[PairingResult]:  # :89-127
    return ParameterCheck("n", N_VALUES, **kw).play()
