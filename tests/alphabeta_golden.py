"""Loader of tests/golden/alphabeta_kats.json (written by tools/make_alphabeta_kats.py from the CPU
restatement tests/c/alphabeta_ref.c) for test_alpha_beta.py and test_gpu_alpha_beta.py."""
import functools
import json
from pathlib import Path

import numpy as np

from onitama_az import _abi

PATH = Path(__file__).resolve().parent / "golden" / "alphabeta_kats.json"
NONE = 255  # move_result: Option::None
INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1


def states(rows) -> np.ndarray:
    a = np.zeros(len(rows), dtype=_abi.STATE_DTYPE)
    for i, (k0, k1, p0, p1, cards, tm) in enumerate(rows):
        a["kings"][i], a["pawns"][i], a["cards"][i], a["to_move"][i] = (k0, k1), (p0, p1), cards, tm
    return a


def moves(rows) -> np.ndarray:
    a = np.zeros(len(rows), dtype=_abi.MOVE_DTYPE)
    for i, m in enumerate(rows):
        a[i] = tuple(m)
    return a


@functools.lru_cache(maxsize=None)
def load() -> dict:
    """The golden file; each search section also as arrays: roots, move (MOVE_DTYPE), score (int32)."""
    d = json.loads(PATH.read_text())
    for key in ("depth4", "depth6"):
        sec = d[key]
        sec["roots"] = states(sec["states"])
        sec["move_np"] = moves(sec["move"])
        sec["score_np"] = np.array(sec["score"], dtype=np.int32)
    return d
