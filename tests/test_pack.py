"""The weight packer on the CPU: csrc/oaz_pack.cpp through the stand-alone tests/c/pack_dump.cpp (no
library, no GPU). Every precision x five weight sets; the packed device image must equal, byte for byte,
what the packer produced before it was moved out of the engine and rewritten against the layout header
(tests/golden/pack_digests.json: SHA-256 of the whole image and of every named section of
csrc/oaz_nn_layout.h).

Regenerate the goldens (only when the layout changes on purpose):
    python tests/test_pack.py --write tests/golden/pack_digests.json [--exe PACK_DUMP]
"""
import hashlib
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
CSRC = ROOT / "onitama-alphazero_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"
DIGESTS = GOLDEN / "pack_digests.json"
PRECISIONS = {"FP32": 0, "BF16": 1, "FP32_SPLIT": 2, "FP32_SPLIT16": 3}
SETS = ("trained3", "trained5", "random0", "random6", "edge3")
CASES = [f"{s}-{p}" for s in SETS for p in PRECISIONS]


def _clangxx():
    """A clang++ with host _Float16 (the packer's fp16 split): ROCm's first, then any on PATH."""
    hipcc = shutil.which("hipcc")
    cands = [Path("/opt/rocm/lib/llvm/bin/clang++")]
    if hipcc:
        cands.append(Path(hipcc).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++")
    for c in cands:
        if c.exists():
            return str(c)
    return shutil.which("clang++")


def build_pack_dump(out_dir: Path) -> Path:
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++ (host _Float16 needs clang)")
    exe = out_dir / "pack_dump"
    # -ffp-contract=off as the library's build: BN folding must not fuse into FMAs
    subprocess.run([cxx, "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(CSRC / "oaz_pack.cpp"), str(ROOT / "tests/c/pack_dump.cpp")], check=True)
    return exe


def edge_weights() -> np.ndarray:
    """The trained 3-block weights with every branch of the scaling / conversion code provoked."""
    from onitama_az.weights import named_from_blob
    blob = np.load(GOLDEN / "weights_3block_trained.npy").copy()
    t = named_from_blob(blob, 3)  # views into blob
    w = t["resnet_0|resnet_small_block1|small_block_conv|weight"]
    w[5] = 0.0                                  # an all-zero output channel (pow2_scale: mx == 0)
    w[7, 3, 1, 1] = 1e30                        # one huge weight in an ordinary channel
    w[9, 0, 0, 0] = 1e-40                       # a subnormal weight
    w[11] = np.ldexp(w[11], -112)               # a channel whose maximum is below 2^-100
    assert 0 < np.abs(w[11]).max() < 2.0 ** -104
    v = t["resnet_2|resnet_small_block2|small_block_conv|weight"]
    v[13, 1, 1, 1] = np.inf                     # a non-finite channel maximum
    v[14, 2, 0, 0] = np.nan                     # NaN (f32_to_bf16's NaN path)
    t["vh_conv|weight"][...] = 0.0              # an all-zero value-head conv
    return blob


def weight_set(name: str):
    if name == "trained3":
        return np.load(GOLDEN / "weights_3block_trained.npy"), 3
    if name == "trained5":
        return np.load(GOLDEN / "weights_5block_trained.npy"), 5
    if name == "edge3":
        return edge_weights(), 3
    from onitama_az.weights import random_weights
    blocks = int(name[len("random"):])
    return random_weights(20260101 + blocks, blocks), blocks


def run_case(exe: Path, work: Path, case: str):
    """(image bytes, packed floats, [(section, offset, length)], blocks, precision) of one case."""
    sname, pname = case.split("-")
    raw_path = work / f"{sname}.f32"
    w, blocks = weight_set(sname)
    if not raw_path.exists():
        np.ascontiguousarray(w, dtype="<f4").tofile(raw_path)
    out = work / f"{case}.bin"
    r = subprocess.run([str(exe), str(raw_path), str(blocks), str(PRECISIONS[pname]), str(out)],
                       capture_output=True, text=True, check=True)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    packed = next(int(ln[1]) for ln in lines if ln[0] == "packed_floats")
    device = next(int(ln[1]) for ln in lines if ln[0] == "device_floats")
    sections = [(ln[1], int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "section"]
    data = out.read_bytes()
    assert len(data) == 4 * device
    return data, packed, sections, blocks, PRECISIONS[pname]


def _sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def pack_dump(tmp_path_factory):
    return build_pack_dump(tmp_path_factory.mktemp("pack_dump"))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("pack_cases")


@pytest.fixture(scope="module")
def digests():
    return json.loads(DIGESTS.read_text())["cases"]


@pytest.mark.parametrize("case", CASES)
def test_packed_image_matches_golden(pack_dump, work, digests, case):
    data, packed, sections, blocks, precision = run_case(pack_dump, work, case)
    gold = digests[case]
    # the sections tile [0, total) in order, no gap, no overlap
    end = 0
    for name, off, length in sections:
        assert off == end and length > 0, f"section {name}: offset {off}, previous end {end}"
        end = off + length
    assert end * 4 == len(data), (end, len(data) // 4)
    assert [s[0] for s in sections] == list(gold["sections"]), "section names / order"
    for name, off, length in sections:
        got = [off, length, _sha(data[4 * off: 4 * (off + length)])]
        assert got == gold["sections"][name], f"first differing section: {name}"
    assert _sha(data) == gold["sha256"]
    from onitama_az import _abi
    if _abi.LIB_PATH.exists():
        assert packed == _abi.load().oaz_nn_device_bytes(blocks, precision) // 4


def main(argv):
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="golden file to write")
    ap.add_argument("--exe", help="a pack_dump to run (default: built from csrc/oaz_pack.cpp)")
    ap.add_argument("--source", default="csrc/oaz_pack.cpp", help="what the packer was built from (header field)")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        exe = Path(a.exe) if a.exe else build_pack_dump(Path(d))
        cases = {}
        for case in CASES:
            data, _packed, sections, blocks, precision = run_case(exe, Path(d), case)
            cases[case] = {"blocks": blocks, "precision": precision, "floats": len(data) // 4, "sha256": _sha(data),
                           "sections": {n: [o, ln, _sha(data[4 * o: 4 * (o + ln)])] for n, o, ln in sections}}
    header = {"packer": a.source, "generator": "python tests/test_pack.py --write tests/golden/pack_digests.json",
              "format": "per case: sha256 of the device image; per section of csrc/oaz_nn_layout.h: "
                        "[offset, length (floats), sha256]"}
    Path(a.write).write_text(json.dumps({"header": header, "cases": cases}, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
