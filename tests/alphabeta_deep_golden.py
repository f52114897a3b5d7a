"""Loader of tests/golden/alphabeta_deep_kats.json (written by tools/make_alphabeta_deep_kats.py from the CPU
restatement tests/c/alphabeta_ref.c) for test_alpha_beta_deep.py and test_gpu_alpha_beta_deep.py."""
import functools
import json
from pathlib import Path

import numpy as np

from alphabeta_golden import moves, states

PATH = Path(__file__).resolve().parent / "golden" / "alphabeta_deep_kats.json"


@functools.lru_cache(maxsize=None)
def load() -> dict:
    """The golden file; depth7 / depth8 also as arrays (roots, move_np, score_np) and `hand_roots`."""
    d = json.loads(PATH.read_text())
    for key in ("depth7", "depth8"):
        sec = d[key]
        sec["roots"] = states(sec["states"])
        sec["move_np"] = moves(sec["move"])
        sec["score_np"] = np.array(sec["score"], dtype=np.int32)
    d["hand_roots"] = states([h["state"] for h in d["hand"]])
    return d
