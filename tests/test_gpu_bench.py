"""GPU: bench.py as a program. A plain run prints one result line for exactly --steps timed steps without the
side measurements, and --dump-outputs writes the last timed ply's outputs, identical from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu
# 8,192 games: above the 4,096 up to which one k_search_grp launch runs a whole ply, so the plies run the
# flagship's per-simulation-step kernels on two game parts; 52 plies, so that games finish and leave samples
G, SIMS, STEPS, WARMUP = 8192, 16, 40, 12
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--games", str(G), "--sims", str(SIMS)]


def test_plain_run_line_and_repeatable_dump(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), *ARGS, "--dump-outputs"]
    runs = [subprocess.Popen(cmd + [str(tmp_path / d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for d in ("a", "b")]  # two fresh processes, side by side
    outs = [p.communicate(timeout=240) for p in runs]
    for p, (_, err) in zip(runs, outs):
        assert p.returncode == 0, err[-2000:]
    lines = outs[0][0].strip().splitlines()
    assert len(lines) == 1, lines  # stdout is the one JSON line
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["game_parts"] == 2 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "sims/s" and d["higher_is_better"] is True and d["dtype"] == "fp32 (fp16x3 split)"
    assert d["ms_per_step"] > 0 and d["checks"]["ok"]
    # the timed region is STEPS plies: every slot searches SIMS simulations per ply (but a root without a legal move)
    timed_sims = d["value"] * d["ms_per_step"] * 1e-3 * d["steps"]
    assert (STEPS - 0.5) * G * SIMS < timed_sims <= STEPS * G * SIMS * (1 + 1e-9)
    for k in ("roofline", "cpu_baseline", "exact_fp32", "leaf_compaction"):  # --full only
        assert k not in d
    assert d["allgather"] is None
    a = {p.name: np.load(p) for p in sorted((tmp_path / "a").glob("*.npy"))}
    b = {p.name: np.load(p) for p in sorted((tmp_path / "b").glob("*.npy"))}
    assert set(a) == set(b) >= {"samples_state.npy", "samples_pi.npy", "samples_z.npy", "tree_root_N.npy"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    # the trees are the last ply's searches: the visits below the root are the ply's simulations (less the one that
    # expanded the root)
    n = a["tree_root_N.npy"].sum(axis=1)
    assert n.max() in (SIMS - 1, SIMS) and np.all((n == n.max()) | (n == 0)) and (n == n.max()).sum() > 0.9 * len(n)
    # the last ply's samples: whole finished games, pi rows normalised, z in {-1, 0, 1}
    assert len(a["samples_pi.npy"]) == int(a["samples_count.npy"][0]) == len(a["samples_z.npy"]) > 0
    assert np.allclose(a["samples_pi.npy"].sum(axis=1), 1.0, atol=1e-5) and set(np.unique(a["samples_z.npy"])) <= {-1.0, 0.0, 1.0}
