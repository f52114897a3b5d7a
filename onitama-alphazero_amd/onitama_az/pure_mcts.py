"""The reference's pure-MCTS agent (onitama-game/src/ai/mcts/mod.rs:13-63) on the GPU.

`Mcts` mirrors the reference struct and Agent impl; every search runs in libonitama_az.so
(oaz_pure_mcts_search: one GPU thread per game, the whole random-rollout UCT search in one
launch). `generate_moves_np` answers a batch of positions at once (the arena's batched fights).

`pure_mcts_search_each` (oaz_pure_mcts_search_each) gives every root its own max_playouts, min_node_visits,
exploration_c and rollout stream in one launch, and has the agent's `search_time` clock on the device;
`Mcts(enforce_search_time=True)` searches through it.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _abi
from .game import DoneMove, GameState


def default_config() -> _abi.oaz_pure_mcts_config:
    cfg = _abi.oaz_pure_mcts_config()
    _abi.load().oaz_pure_mcts_config_default(C.byref(cfg))
    return cfg


@dataclass
class PureSearchResult:
    moves: np.ndarray                 # [G] MOVE_DTYPE (from == 25: pass)
    values: np.ndarray                # [G] float32 winrate of the chosen child
    stats: _abi.oaz_pure_mcts_stats
    trees: Optional[np.ndarray]       # [G, cap] PURE_NODE_DTYPE when requested (search_each: packed, [offsets[G]])
    playouts: Optional[np.ndarray] = None  # search_each: [G] int32, the playouts each root ran
    offsets: Optional[np.ndarray] = None   # search_each with trees: [G + 1], root g's nodes = trees[offsets[g]:offsets[g + 1]]

    def tree(self, g: int) -> np.ndarray:
        """Root g's nodes, up to its capacity."""
        return self.trees[g] if self.offsets is None else self.trees[int(self.offsets[g]): int(self.offsets[g + 1])]


def pure_mcts_search(roots: np.ndarray, max_playouts: int = 5000, min_node_visits: int = 5,
                     exploration_c: float = math.sqrt(2.0), seed: int = 20260101, game_id0: int = 0,
                     rollout_cap: int = 1000, with_trees: bool = False, device: int = 0) -> PureSearchResult:
    roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE).reshape(-1)
    cfg = default_config()
    cfg.max_playouts, cfg.min_node_visits = int(max_playouts), int(min_node_visits)
    cfg.exploration_c, cfg.seed, cfg.game_id0, cfg.rollout_cap = float(exploration_c), seed, game_id0, rollout_cap
    cfg.device = int(device)
    lib = _abi.load()
    G = len(roots)
    moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
    values = np.zeros(G, dtype=np.float32)
    st = _abi.oaz_pure_mcts_stats()
    cap = int(lib.oaz_pure_mcts_tree_capacity(C.byref(cfg))) if with_trees else 0
    trees = np.zeros((G, cap), dtype=_abi.PURE_NODE_DTYPE) if with_trees else None
    _abi.check(lib.oaz_pure_mcts_search(_abi.ptr(roots), G, C.byref(cfg), _abi.ptr(moves), _abi.ptr(values),
                                        C.byref(st), _abi.ptr(trees) if with_trees else None, cap))
    return PureSearchResult(moves, values, st, trees)


def root_params(G: int, max_playouts, min_node_visits, exploration_c, streams) -> np.ndarray:
    """[G] PURE_ROOT_DTYPE (oaz_pure_mcts_root) from scalars or length-G arrays."""
    par = np.zeros(G, dtype=_abi.PURE_ROOT_DTYPE)
    for name, v in (("max_playouts", max_playouts), ("min_node_visits", min_node_visits),
                    ("exploration_c", exploration_c), ("stream", streams)):
        par[name] = np.broadcast_to(np.asarray(v), (G,))
    return par


def pure_mcts_search_each(roots: np.ndarray, max_playouts=5000, min_node_visits=5, exploration_c=math.sqrt(2.0),
                          streams=0, seed: int = 20260101, rollout_cap: int = 1000, search_time: Optional[float] = None,
                          with_trees: bool = False, device: int = 0) -> PureSearchResult:
    """One search per root, root g with its own max_playouts, min_node_visits, exploration_c and rollout stream
    (scalars or length-G arrays): each answer is pure_mcts_search's on that root alone with game_id0 = its stream.
    search_time in seconds is the reference's clock on the device (every root runs at least
    min(max_playouts, min_node_visits + 2) playouts); None or 0 runs exactly max_playouts. `playouts` are the
    playouts each root ran; with_trees returns the trees packed by `offsets`."""
    roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE).reshape(-1)
    G = len(roots)
    par = root_params(G, max_playouts, min_node_visits, exploration_c, streams)
    cfg = _abi.oaz_pure_mcts_each_config()
    cfg.seed, cfg.rollout_cap, cfg.device = int(seed), int(rollout_cap), int(device)
    cfg.search_time_ns = 0 if search_time is None else int(round(float(search_time) * 1e9))
    lib = _abi.load()
    moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
    values = np.zeros(G, dtype=np.float32)
    playouts = np.zeros(G, dtype=np.int32)
    st = _abi.oaz_pure_mcts_stats()
    offsets = trees = None
    if with_trees:
        offsets = np.zeros(G + 1, dtype=np.uintp)
        total = int(lib.oaz_pure_mcts_each_capacity(_abi.ptr(par), G, _abi.ptr(offsets)))
        trees = np.zeros(total, dtype=_abi.PURE_NODE_DTYPE)
    _abi.check(lib.oaz_pure_mcts_search_each(_abi.ptr(roots), _abi.ptr(par), G, C.byref(cfg), _abi.ptr(moves),
                                             _abi.ptr(values), _abi.ptr(playouts), C.byref(st),
                                             _abi.ptr(trees) if with_trees else None,
                                             _abi.ptr(offsets) if with_trees else None))
    return PureSearchResult(moves, values, st, trees, playouts, offsets)


def release_workspace(device: int = 0) -> None:
    """Free the device buffer the searches on `device` keep between calls (oaz_pure_mcts_release_workspace)."""
    _abi.check(_abi.load().oaz_pure_mcts_release_workspace(int(device)))


@dataclass
class Mcts:  # ai/mcts/mod.rs:13-30
    """With the defaults every search runs exactly max_playouts and search_time is kept for id() only.
    enforce_search_time=True is the reference's clock (search_time seconds per search, read on the device,
    pure_mcts_search_each); with a budget that does not bind the moves are the same."""
    search_time: float = 1.0
    min_node_visits: int = 5
    exploration_c: float = math.sqrt(2.0)
    max_playouts: int = 5000
    seed: int = 20260101
    device: int = 0  # the GPU the searches run on (common.rs Options.device)
    enforce_search_time: bool = False

    def __post_init__(self):
        self._calls = 0

    def generate_move(self, game_state: GameState) -> Tuple[DoneMove, float]:  # mod.rs:37-52
        r = self._search(game_state.state.to_np(game_state.curr_player_color))
        return DoneMove.from_c(r.moves[0]), float(r.values[0])

    def generate_moves_np(self, roots: np.ndarray) -> np.ndarray:
        return self._search(roots).moves

    def _search(self, roots: np.ndarray) -> PureSearchResult:
        # a fresh rollout stream per call (the reference draws from thread_rng)
        g0 = self._calls << 20
        self._calls += 1
        if self.enforce_search_time:
            return pure_mcts_search_each(roots, self.max_playouts, self.min_node_visits, self.exploration_c,
                                         g0 + np.arange(np.asarray(roots).size, dtype=np.uint64), self.seed,
                                         search_time=self.search_time, device=self.device)
        return pure_mcts_search(roots, self.max_playouts, self.min_node_visits, self.exploration_c, self.seed, g0,
                                device=self.device)

    def reserve(self, n: int) -> None:
        pass

    def device_key(self):  # a stateless GPU search (its own buffers and stream per call): may run beside an engine's
        return ("pure_mcts", id(self))

    def name(self) -> str:
        return "MCTS AI"

    def id(self) -> int:  # mod.rs:57-62
        return (int(self.search_time * 1e9) + int(self.exploration_c) + self.max_playouts + self.min_node_visits)
