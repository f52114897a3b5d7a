"""The held-out split: which records are kept out of training, as a function of the position alone
(oaz_holdout_*; the rule is stated in include/onitama_az.h, "held-out evaluation", and DESIGN.md section 5j).
All copies of a position, in every iteration of a replay window, fall on the same side, and so does a merged
record. This module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import _abi


def pick(state: np.ndarray, seed: int, per_65536: int) -> bool:
    """One position (a STATE_DTYPE record) on the host: oaz_holdout_pick."""
    s = np.ascontiguousarray(state, dtype=_abi.STATE_DTYPE).reshape(1)
    rc = _abi.load().oaz_holdout_pick(C.c_uint64(int(seed)), _abi.ptr(s), int(per_65536))
    _abi.check(rc)
    return bool(rc)


def mask(samples, seed: int, per_65536: int, device: int = 0) -> np.ndarray:
    """uint8 [n], 1 = held out, with the share per_65536 / 65 536 of the positions. samples: a SAMPLE_DTYPE array
    (the rule on the host, oaz_holdout_mask_host, no GPU), or (device pointer, n) of records in the memory of
    `device` (a ReplayBuffer view; a kernel over them, oaz_holdout_mask: they do not move)."""
    lib = _abi.load()
    if isinstance(samples, tuple):
        ptr, n = int(samples[0]), int(samples[1])
        out = np.zeros(n, dtype=np.uint8)
        _abi.check(lib.oaz_holdout_mask(C.c_void_p(ptr), n, C.c_uint64(int(seed)), int(per_65536), int(device),
                                        _abi.ptr(out)))
        return out
    samples = np.ascontiguousarray(samples, dtype=_abi.SAMPLE_DTYPE)
    out = np.zeros(len(samples), dtype=np.uint8)
    _abi.check(lib.oaz_holdout_mask_host(_abi.ptr(samples), len(samples), C.c_uint64(int(seed)), int(per_65536),
                                         _abi.ptr(out)))
    return out


def split(mask: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(train_ids, holdout_ids) of a mask: both ascending int32."""
    m = np.asarray(mask).reshape(-1) != 0
    return np.nonzero(~m)[0].astype(np.int32), np.nonzero(m)[0].astype(np.int32)
