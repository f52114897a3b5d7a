"""ReplayBuffer: the training data of the last `window` iterations, kept on the device, with a merged view in
which records of equal position are one record with the mean pi and the mean z (oaz_replay_*,
csrc/oaz_replay.hip; the rule is stated in include/onitama_az.h, "replay buffer", and DESIGN.md section 5h).

The reference keeps one iteration's Vec (train.rs:241-250) and trains on every copy; LoopConfig's defaults do
too. This module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _abi


def merge_host(samples: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(merged records, multiplicities uint32) by the merge rule on the host (oaz_replay_merge_host; no GPU)."""
    samples = np.ascontiguousarray(samples, dtype=_abi.SAMPLE_DTYPE)
    out = np.zeros(len(samples), dtype=_abi.SAMPLE_DTYPE)
    mult = np.zeros(len(samples), dtype=np.uint32)
    n = C.c_size_t(0)
    _abi.check(_abi.load().oaz_replay_merge_host(_abi.ptr(samples), len(samples), _abi.ptr(out), _abi.ptr(mult),
                                                 C.byref(n)))
    return out[: n.value].copy(), mult[: n.value].copy()


class ReplayBuffer:
    """capacity: records (LoopConfig.buffer_size); window: appends (iterations) kept; table_slots: the merge's key
    table, 0 = the smallest power of two >= 2 n, else a power of two above the records of the view being built."""

    def __init__(self, capacity: int = 180_000, window: int = 1, device: int = 0, table_slots: int = 0):
        lib = _abi.load()
        cfg = _abi.oaz_replay_config()
        lib.oaz_replay_config_default(C.byref(cfg))
        cfg.capacity, cfg.window, cfg.device, cfg.table_slots = int(capacity), int(window), int(device), int(table_slots)
        h = lib.oaz_replay_create(C.byref(cfg))
        if not h:
            raise _abi.OazError(f"oaz_replay_create failed: {lib.oaz_last_error().decode()}")
        self._h, self._lib, self.config, self.device = C.c_void_p(h), lib, cfg, int(device)

    def close(self) -> None:
        if self._h:
            self._lib.oaz_replay_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- one segment per call ------------------------------------------------------------------
    def append(self, samples: np.ndarray, tag: int = 0) -> None:
        samples = np.ascontiguousarray(samples, dtype=_abi.SAMPLE_DTYPE)
        _abi.check(self._lib.oaz_replay_append_host(self._h, _abi.ptr(samples), len(samples), int(tag)))

    def append_device(self, ptr: int, n: int, tag: int = 0) -> None:
        _abi.check(self._lib.oaz_replay_append_device(self._h, C.c_void_p(ptr), int(n), int(tag)))

    def append_engine(self, eng, tag: int = 0) -> int:
        """All of the engine's buffered samples, device to device; returns how many."""
        n = C.c_size_t(0)
        _abi.check(self._lib.oaz_replay_append_engine(self._h, eng._h, int(tag), C.byref(n)))
        return int(n.value)

    # -- the window ----------------------------------------------------------------------------
    def view(self, merge: bool = False) -> Tuple[int, int, Optional[int]]:
        """(device pointer, records, device pointer of the uint32 multiplicities or None): valid until the next
        append, view, fetch or close."""
        p, m, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        _abi.check(self._lib.oaz_replay_view(self._h, int(bool(merge)), C.byref(p), C.byref(n), C.byref(m)))
        return int(p.value or 0), int(n.value), (int(m.value) if m.value else None)

    def fetch(self, merge: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The view on the host: (records, multiplicities; all 1 without merging)."""
        cap = int(self.stats().records)
        out = np.zeros(cap, dtype=_abi.SAMPLE_DTYPE)
        mult = np.zeros(cap, dtype=np.uint32)
        n = C.c_size_t(0)
        _abi.check(self._lib.oaz_replay_fetch(self._h, int(bool(merge)), _abi.ptr(out), _abi.ptr(mult), cap, C.byref(n)))
        return out[: n.value], mult[: n.value]

    def stats(self) -> _abi.oaz_replay_stats:
        st = _abi.oaz_replay_stats()
        _abi.check(self._lib.oaz_replay_stats_get(self._h, C.byref(st)))
        return st

    def merge_times(self) -> dict:
        """The last merged view's device milliseconds by phase (_abi.REPLAY_PHASES)."""
        ms = (C.c_double * len(_abi.REPLAY_PHASES))()
        _abi.check(self._lib.oaz_replay_merge_times(self._h, C.byref(ms)))
        return dict(zip(_abi.REPLAY_PHASES, (float(x) for x in ms)))

    merge_host = staticmethod(merge_host)
