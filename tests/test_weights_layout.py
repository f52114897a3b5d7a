"""The canonical weight blob's one statement, csrc/oaz_weights_layout.h, on the CPU: the stand-alone
tests/c/weights_layout_dump.cpp (the header alone: no library, no GPU) prints the tensor table, the
total, the BN-statistics segments and the SGD mask's runs, and everything is compared with values
computed here from the independent restatement onitama_az.weights.canonical_layout."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))

from onitama_az import weights as W  # noqa: E402
from test_pack import _clangxx  # noqa: E402

BLOCKS = (0, 1, 3, 5, 6, 16)
PINNED_TOTALS = {3: 240_006, 5: 388_742, 6: 463_110}  # SURVEY.md, as tests/test_host.py pins them


@pytest.fixture(scope="module")
def layout_dump(tmp_path_factory):
    cxx = _clangxx() or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("weights_layout_dump") / "weights_layout_dump"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(ROOT / "tests/c/weights_layout_dump.cpp")],
                   check=True)
    return exe


def dump(exe, *args):
    """(tensors [(name, shape, offset, numel, running_stat)], total, segments [(offset, len)], mask runs
    [(value, offset, len)]) as the header states them."""
    out = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout
    lines = [ln.split() for ln in out.splitlines()]
    tensors = [(ln[1], tuple(int(d) for d in ln[2].split(",")), int(ln[3]), int(ln[4]), bool(int(ln[5])))
               for ln in lines if ln[0] == "tensor"]
    total = next(int(ln[1]) for ln in lines if ln[0] == "total")
    segs = [(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == "bn_segment"]
    runs = [(int(ln[1]), int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "sgd_run"]
    return tensors, total, segs, runs


@pytest.mark.parametrize("blocks", BLOCKS)
def test_layout_equals_python_restatement(layout_dump, blocks):
    tensors, total, segs, runs = dump(layout_dump, blocks)
    ref = W.canonical_layout(blocks)
    assert [t[0] for t in tensors] == [n for n, _ in ref], "names / creation order"
    assert [t[1] for t in tensors] == [tuple(s) for _, s in ref], "shapes"
    numel = [int(np.prod(s)) for _, s in ref]
    offsets = [int(o) for o in np.concatenate([[0], np.cumsum(numel)[:-1]])]
    assert [t[3] for t in tensors] == numel
    assert [t[2] for t in tensors] == offsets, "offsets are the running sum"
    assert total == W.weight_count(blocks) == sum(numel)
    if blocks in PINNED_TOTALS:
        assert total == PINNED_TOTALS[blocks]
    # running statistics: exactly the running_mean / running_var tensors
    assert [t[4] for t in tensors] == [n.endswith(("running_mean", "running_var")) for n, _ in ref]
    at = {n: o for (n, _), o in zip(ref, offsets)}
    convs = ["bn1"] + [f"resnet_{i}|resnet_small_block{j}|small_block_bn" for i in range(blocks) for j in (1, 2)]
    # pack order of oaz_trainer_bn_stats_pack: per conv layer mean + var (adjacent: one segment of 128), then
    # the value head's 1 + 1 and the policy head's 2 + 2
    want = [(at[f"{bn}|running_mean"], 128) for bn in convs]
    want += [(at["vh_bn|running_mean"], 2), (at["policy_bn|running_mean"], 4)]
    assert segs == want
    for bn in convs + ["vh_bn", "policy_bn"]:  # (adjacent indeed: var follows mean)
        assert at[f"{bn}|running_var"] == at[f"{bn}|running_mean"] + (64 if bn in convs else 1 if bn == "vh_bn" else 2)
    flagged = sum(t[3] for t in tensors if t[4])
    assert flagged == sum(ln for _, ln in segs) == (1 + 2 * blocks) * 128 + 6
    # SGD mask: 0 on the running statistics, 1 elsewhere; its runs tile [0, total)
    mask = np.ones(total, dtype=np.uint8)
    for (n, _), o, k in zip(ref, offsets, numel):
        if n.endswith(("running_mean", "running_var")):
            mask[o:o + k] = 0
    edges = np.concatenate([[0], np.nonzero(np.diff(mask))[0] + 1, [total]])
    assert runs == [(int(mask[a]), int(a), int(b - a)) for a, b in zip(edges[:-1], edges[1:])]
    assert [(o, ln) for v, o, ln in runs if v == 0] == segs


def test_total_at_a_non_default_shape(layout_dump):
    """layout(2, 32, 10): the closed formula the library had before the header (tower first layer, two
    blocks, value head, policy head)."""
    C, I, blocks = 32, 10, 2
    _, total, _, _ = dump(layout_dump, blocks, C, I)
    first = C * I * 9 + C + 4 * C
    tower = blocks * 2 * (C * C * 9 + C + 4 * C)
    value = C + 1 + 4 + C * 25 + C + C + 1
    policy = 2 * C + 2 + 8 + 50 * 50 + 50
    assert (first, tower, value, policy) == (3040, 37504, 902, 2624)
    assert total == 44_070 == first + tower + value + policy
