"""Engine: owner of one oaz_engine (one GPU) — batched NN, search and self-play."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _abi


@dataclass
class SearchResult:
    moves: np.ndarray        # [G] MOVE_DTYPE
    pi: np.ndarray           # [G, 2, 25] float32
    root_value: Optional[np.ndarray]  # [G] float32 (extra root evaluation)
    stats: _abi.oaz_search_stats
    roots: Optional[np.ndarray] = None  # [G] STATE_DTYPE: the positions searched (Engine.resume only)


def playout_cap_full(seed: int, game_id: int, ply: int, full_per_65536: int) -> bool:
    """The playout cap rule on the host (oaz_playout_cap_full; no device): whether ply `ply` of global game
    `game_id` under `seed` is a full ply when full_per_65536 of 65 536 plies are."""
    rc = _abi.load().oaz_playout_cap_full(int(seed), int(game_id), int(ply), int(full_per_65536))
    _abi.check(rc)
    return bool(rc)


class Engine:
    """One engine on one GPU. Mirrors the state a reference worker thread owns (a model copy
    and its searches, train.rs:218-238) but for `games` games at once."""

    def __init__(self, config: Optional[_abi.oaz_config] = None, device: int = 0, **overrides):
        lib = _abi.load()
        cfg = config if config is not None else _abi.default_config()
        playout_cap = overrides.pop("playout_cap", None)  # (fast_sims, full_per_65536): an engine setting, not a field
        for k, v in overrides.items():
            if k == "deck":
                for i, c in enumerate(v):
                    cfg.deck[i] = int(c)
            else:
                setattr(cfg, k, v)
        self.config = cfg
        h = lib.oaz_create(C.byref(cfg), int(device))
        if not h:
            raise _abi.OazError(f"oaz_create failed: {lib.oaz_last_error().decode()}")
        self._h = C.c_void_p(h)
        self._lib = lib
        self.device = device
        if playout_cap is not None:
            try:
                self.set_playout_cap(*playout_cap)
            except Exception:
                self.close()
                raise

    # -- lifecycle --
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.oaz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def load_weights(self, blob: np.ndarray) -> None:
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        _abi.check(self._lib.oaz_load_weights(self._h, _abi.ptr(blob), blob.size))

    def set_search_params(self, sims: int, c_puct: float, train_noise: bool) -> None:
        """Per-agent AlphaZeroMctsConfig for the next searches (sims <= the creation budget)."""
        _abi.check(self._lib.oaz_set_search_params(self._h, int(sims), float(c_puct), int(bool(train_noise))))

    def set_search_time(self, seconds: float) -> None:
        """Q7 wall-clock budget per search / ply (AlphaZeroMctsConfig.search_time); 0 = off (exactly
        `sims` playouts, the parity mode)."""
        _abi.check(self._lib.oaz_set_search_time(self._h, int(round(float(seconds) * 1e9))))

    def last_sims(self) -> int:
        """Simulations per game of the last search / ply (< sims when a search_time budget stopped it)."""
        n = C.c_int(0)
        _abi.check(self._lib.oaz_last_sims(self._h, C.byref(n)))
        return int(n.value)

    def search_playouts(self, games: int) -> np.ndarray:
        """Playouts each of the first `games` games of the last search ran (a device-side search_time
        budget stops every game, or 16-game group, on its own clock read)."""
        out = np.zeros(int(games), dtype=np.int32)
        _abi.check(self._lib.oaz_search_playouts(self._h, _abi.ptr(out), int(games)))
        return out

    def leaf_batch_stats(self) -> Tuple[int, int, int]:
        """Engine(leaf_batch=L), L = 1 .. 16 (the leaf-parallel search: up to L leaves of a root's tree per network
        pass, virtual loss): (rounds, playouts, discarded walks) of the last search, summed over its roots; all 0
        with leaf_batch = 0."""
        out = (C.c_uint64 * 3)()
        _abi.check(self._lib.oaz_search_leaf_batch_stats(self._h, C.byref(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def sync(self) -> None:
        _abi.check(self._lib.oaz_sync(self._h))

    # -- NN --
    def nn_forward(self, states: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """ConvResNet::forward(train=false) (net.rs:215-232): policy [B,2,25], value [B]."""
        states = np.ascontiguousarray(states, dtype=_abi.STATE_DTYPE)
        B = len(states)
        pol = np.zeros((B, 2, 25), dtype=np.float32)
        val = np.zeros(B, dtype=np.float32)
        _abi.check(self._lib.oaz_nn_forward(self._h, _abi.ptr(states), B, _abi.ptr(pol), _abi.ptr(val)))
        return pol, val

    def nn_fallbacks(self) -> int:
        """OAZ_FP32_SPLIT16: 16-position tiles recomputed with the bf16x6 split (fp16 range)."""
        n = C.c_uint64(0)
        _abi.check(self._lib.oaz_nn_fallbacks(self._h, C.byref(n)))
        return int(n.value)

    # -- search --
    def search(self, roots: np.ndarray, root_value: bool = False) -> SearchResult:
        roots = np.ascontiguousarray(roots, dtype=_abi.STATE_DTYPE)
        G = len(roots)
        moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
        pi = np.zeros((G, 2, 25), dtype=np.float32)
        rv = np.zeros(G, dtype=np.float32) if root_value else None
        st = _abi.oaz_search_stats()
        _abi.check(self._lib.oaz_search(self._h, _abi.ptr(roots), G, _abi.ptr(moves), _abi.ptr(pi),
                                        _abi.ptr(rv) if rv is not None else None, C.byref(st)))
        return SearchResult(moves, pi, rv, st)

    def tree(self, game: int) -> np.ndarray:
        n = C.c_int(0)
        _abi.check(self._lib.oaz_tree_dump(self._h, game, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=_abi.NODE_DTYPE)
        _abi.check(self._lib.oaz_tree_dump(self._h, game, _abi.ptr(out), n.value, C.byref(n)))
        return out

    # -- tree reuse (Engine(reuse_visits=R), R >= sims: a tree's capacity in root visits) --
    def advance(self, moves: np.ndarray) -> np.ndarray:
        """Re-roots the trees of the last search / resume at moves[g] and steps the engine's resident roots by
        them. Returns kept [G] int32: the visits of the kept subtree's root, 0 where the game got a fresh tree
        (the keep rule, oaz_config.reuse_visits)."""
        moves = np.ascontiguousarray(moves, dtype=_abi.MOVE_DTYPE)
        kept = np.zeros(len(moves), dtype=np.int32)
        _abi.check(self._lib.oaz_search_advance(self._h, _abi.ptr(moves), len(moves), _abi.ptr(kept)))
        return kept

    def resume(self, G: int, root_value: bool = False) -> SearchResult:
        """`sims` more playouts on the first G trees as advance() left them, from the resident roots
        (returned as SearchResult.roots)."""
        G = int(G)
        moves = np.zeros(G, dtype=_abi.MOVE_DTYPE)
        pi = np.zeros((G, 2, 25), dtype=np.float32)
        rv = np.zeros(G, dtype=np.float32) if root_value else None
        roots = np.zeros(G, dtype=_abi.STATE_DTYPE)
        st = _abi.oaz_search_stats()
        _abi.check(self._lib.oaz_search_resume(self._h, G, _abi.ptr(moves), _abi.ptr(pi),
                                               _abi.ptr(rv) if rv is not None else None, C.byref(st), _abi.ptr(roots)))
        return SearchResult(moves, pi, rv, st, roots)

    def reuse_stats(self) -> _abi.oaz_reuse_stats:
        st = _abi.oaz_reuse_stats()
        _abi.check(self._lib.oaz_reuse_stats_get(self._h, C.byref(st)))
        return st

    # -- self-play temperature (Engine(temperature_plies=T): a game's first T plies draw the move from the visits) --
    def sample_moves(self, game_ids, plies) -> Tuple[np.ndarray, np.ndarray]:
        """After search() / resume(): (moves [G] MOVE_DTYPE, child [G] int32) the temperature rule draws from
        game g's tree for (game_ids[g], plies[g]) under the engine's seed, whatever temperature_plies is: the
        drawn child, the most visited one where no child has a visit, the pass move and child -1 without a child."""
        game_ids = np.ascontiguousarray(game_ids, dtype=np.uint64)
        plies = np.ascontiguousarray(plies, dtype=np.uint32)
        if game_ids.shape != plies.shape or game_ids.ndim != 1:
            raise ValueError("sample_moves: game_ids and plies are two 1-d arrays of one length")
        moves = np.zeros(len(game_ids), dtype=_abi.MOVE_DTYPE)
        child = np.zeros(len(game_ids), dtype=np.int32)
        _abi.check(self._lib.oaz_search_sample_moves(self._h, len(game_ids), _abi.ptr(game_ids), _abi.ptr(plies),
                                                     _abi.ptr(moves), _abi.ptr(child)))
        return moves, child

    def temperature_stats(self) -> Tuple[int, int]:
        """(self-play plies whose move was drawn, draws whose child is not the most visited one) since
        selfplay_reset()."""
        out = (C.c_uint64 * 2)()
        _abi.check(self._lib.oaz_selfplay_temperature_stats(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    # -- playout cap randomization (Engine(playout_cap=(n, P)): a random share P / 65 536 of the plies is searched with
    # `sims` playouts and recorded, the others with n playouts and only played) --
    def set_playout_cap(self, fast_sims: int, full_per_65536: int = 16384) -> None:
        """The cap for the following self-play (fast_sims = 0: off). Ends the running games: the next
        selfplay_step() starts from a reset. Refused (OazError) on an engine with tree reuse, leaf batching or a
        search-time budget."""
        _abi.check(self._lib.oaz_selfplay_set_playout_cap(self._h, int(fast_sims), int(full_per_65536)))

    def playout_cap_stats(self) -> Tuple[int, int]:
        """(full plies, fast plies) played since selfplay_reset(); (0, 0) without a cap."""
        out = (C.c_uint64 * 2)()
        _abi.check(self._lib.oaz_selfplay_playout_cap_stats(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    # -- self-play --
    def selfplay_reset(self) -> None:
        _abi.check(self._lib.oaz_selfplay_reset(self._h))

    def selfplay_step(self, moves: int = 1) -> None:
        _abi.check(self._lib.oaz_selfplay_step(self._h, int(moves)))

    def selfplay_stats(self) -> _abi.oaz_selfplay_stats:
        st = _abi.oaz_selfplay_stats()
        _abi.check(self._lib.oaz_selfplay_stats_get(self._h, C.byref(st)))
        return st

    def samples_fetch(self, cap: int) -> np.ndarray:
        out = np.zeros(cap, dtype=_abi.SAMPLE_DTYPE)
        n = C.c_size_t(0)
        _abi.check(self._lib.oaz_samples_fetch(self._h, _abi.ptr(out), cap, C.byref(n)))
        return out[: n.value]

    def samples_export_device(self, dev_ptr: int, cap_bytes: int) -> int:
        n = C.c_size_t(0)
        _abi.check(self._lib.oaz_samples_export_device(self._h, C.c_void_p(dev_ptr), cap_bytes, C.byref(n)))
        return n.value

    def selfplay_run(self, n_games: int, cap: int) -> Tuple[np.ndarray, _abi.oaz_selfplay_stats]:
        out = np.zeros(cap, dtype=_abi.SAMPLE_DTYPE)
        n = C.c_size_t(0)
        st = _abi.oaz_selfplay_stats()
        _abi.check(self._lib.oaz_selfplay_run(self._h, int(n_games), _abi.ptr(out), cap, C.byref(n), C.byref(st)))
        return out[: n.value], st

    # -- timing --
    def set_timing(self, on) -> None:
        """False/True: off / every launch; an int N > 1: the kernels of every N-th simulation step."""
        _abi.check(self._lib.oaz_set_timing(self._h, int(on) if not isinstance(on, bool) else (1 if on else 0)))

    def kernel_times(self) -> _abi.oaz_kernel_times:
        t = _abi.oaz_kernel_times()
        _abi.check(self._lib.oaz_kernel_times_get(self._h, C.byref(t)))
        return t

    def kernel_times_reset(self) -> None:
        _abi.check(self._lib.oaz_kernel_times_reset(self._h))
