"""The four agents against each other: alphazero-training/src/bin/tournament.rs.

`Tournament.pit()` plays the reference's six pairings in its order (AlphaBeta-Mcts, AlphaBeta-AlphaZero,
AlphaBeta-Random, Mcts-AlphaZero, Mcts-Random, AlphaZero-Random) over one list of decks: game k of every
pairing is dealt oaz_deal_deck(seed, k) (the reference draws `game_amnt` decks once, tournament.rs:89-92).
A pairing is one batched `evaluator.fight` (the first-named agent plays Red in even games, `agents.swap`,
tournament.rs:65-66), whose results are folded in game order by `fold_pairing`: the four ratings start at 800
and are carried from pairing to pairing, a win or a loss goes through oaz_elo_change and anything else changes
nothing (tournament.rs:54-63).

Defined where the reference is not: it re-plays a game cut by the ply budget (`game -= 1`, tournament.rs:44-48,
which underflows at game 0). Here a cut game is a no-result: it is counted (`cut`), changes no rating, counts
as a game in the winrate's denominator (the reference divides by game_amnt) and is not replayed.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

from . import _abi
from .evaluator import AlphaZeroAgent, EvaluatorConfig, fight
from .game import Deck

PAIRINGS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # tournament.rs:136-188 over AGENTS
AGENTS = ("alphabeta", "mcts", "alphazero", "random")
START_RATING = 800.0  # tournament.rs:84-87


def fold_pairing(results: Sequence[int], rating_a: float, rating_b: float) -> Tuple[float, float, int, int]:
    """tournament.rs:54-68 over a pairing's last MoveResult codes in game order, the first-named agent playing
    Red in even games: (rating_a, rating_b, its wins, the games without a winner)."""
    lib = _abi.load()
    ra, rb = C.c_double(rating_a), C.c_double(rating_b)
    wins = cut = 0
    for k, r in enumerate(results):
        mine, theirs = (_abi.RED_WIN, _abi.BLUE_WIN) if k % 2 == 0 else (_abi.BLUE_WIN, _abi.RED_WIN)
        if r == mine or r == theirs:
            wins += r == mine
            lib.oaz_elo_change(ra.value, rb.value, int(r == mine), C.byref(ra), C.byref(rb))
        else:
            cut += 1
    return ra.value, rb.value, wins, cut


@dataclass
class PairingResult:
    agent: str                  # the keys of Tournament.agents
    opponent: str
    results: List[int]          # every game's last MoveResult
    plies: List[int]
    wins: int                   # of the first-named agent
    cut: int                    # games ended by the ply budget: no result
    winrate: float              # wins / game_amnt (tournament.rs:76)
    ratings: dict               # all four ratings after this pairing
    elapsed_s: float
    decks: List[List[int]] = field(default_factory=list)  # the pairing's deals: the tournament's


def default_agents(model, seed: int = 20260101, device: int = 0, leaf_batch: int = 0) -> dict:
    """tournament.rs:107-134: AlphaBeta{8, 1 s}, Mcts{1 s, min visits 0, c 1.0, 5 000 playouts},
    AlphaZeroMcts{1 s, c 1.0, 5 000 playouts, no noise} on `model` (a ConvResNet), Random. leaf_batch: the
    AlphaZero agent's AlphaZeroMctsConfig.leaf_batch (0: the reference's sequential search; L > 0 searches at most
    CU-count games per ply, i.e. game_amnt <= the device's CU count)."""
    from .alpha_beta import AlphaBeta
    from .arena import NativeRandomAgent
    from .mcts import AlphaZeroMctsConfig
    from .pure_mcts import Mcts
    return {
        "alphabeta": AlphaBeta(max_depth=8, search_time=1.0, device=device, enforce_search_time=True),
        "mcts": Mcts(search_time=1.0, min_node_visits=0, exploration_c=1.0, max_playouts=5000, seed=seed, device=device),
        "alphazero": AlphaZeroAgent(AlphaZeroMctsConfig(search_time=1.0, exploration_c=1.0, max_playouts=5000,
                                                        train=False, leaf_batch=leaf_batch), model),
        "random": NativeRandomAgent(seed),
    }


class Tournament:
    """bin/tournament.rs `pit`. The agents are what `evaluator.fight` takes (generate_moves_np, name, reserve);
    see default_agents for the reference's four. `play` is the fight (evaluator.fight by default); `play=functools.partial(arena.native_fight, slots=S)`
    plays every pairing on a pool of S refilled game slots, with the AlphaZero engine sized for S."""

    def __init__(self, alphabeta, mcts, alphazero, random, game_amnt: int = 100, max_plies: int = 150,
                 seed: int = 20260101, play: Optional[Callable] = None, verbose: bool = True):
        self.agents = dict(zip(AGENTS, (alphabeta, mcts, alphazero, random)))
        self.game_amnt, self.max_plies, self.seed = int(game_amnt), int(max_plies), int(seed)
        self.play = play if play is not None else fight
        self.verbose = verbose
        self.ratings = {k: START_RATING for k in AGENTS}
        self.decks = [[int(c) for c in Deck.default(self.seed, k).indices()] for k in range(self.game_amnt)]

    def pit(self) -> List[PairingResult]:
        out = []
        for a, b in ((AGENTS[i], AGENTS[j]) for i, j in PAIRINGS):
            t0 = time.perf_counter()
            config = EvaluatorConfig(game_amnt=self.game_amnt, deck=None, max_plies=self.max_plies, seed=self.seed)
            st = self.play(config, self.agents[a], self.agents[b])
            ra, rb, wins, cut = fold_pairing(st.results, self.ratings[a], self.ratings[b])
            self.ratings[a], self.ratings[b] = ra, rb
            dt = time.perf_counter() - t0
            winrate = wins / self.game_amnt if self.game_amnt else float("nan")
            out.append(PairingResult(a, b, list(st.results), list(st.plies), wins, cut, winrate, dict(self.ratings), dt,
                                     self.decks))
            if self.verbose:  # tournament.rs:70-78
                print(f"{self.agents[a].name()} ({ra:5.2f}) vs {self.agents[b].name()} ({rb:5.2f}) -> "
                      f"winrate: {winrate:3.2f}")
                print(f"Elapsed: {dt:.3f}s\n")
        return out
