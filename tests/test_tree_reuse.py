"""CPU: tree reuse without a device. The host restatement of the device's re-rooting (oaz_tree_rebase_host; the
compaction is stated once, in csrc/oaz_tree_rebase.h) against the oracle's fresh searches, its error cases, the
ABI of the new setting and entry points, and a plain C program under the address and undefined-behaviour
sanitizers. The invariant (DESIGN.md "Tree reuse"): the subtree of a visited root child c, taken out with its
node order kept, equals the oracle's fresh search of N_c playouts from c's position, node for node."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from onitama_az import _abi
from tree_reuse_util import assert_trees_equal, stepped, unpack, usable_roots

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "onitama-alphazero_amd" / "csrc"
CASES = [(33, 1.4), (64, 5.0), (200, 2.0)]


def rebase_host(lib, nodes, child, cap=None):
    nodes = np.ascontiguousarray(nodes)
    cap = len(nodes) if cap is None else cap
    out = np.frombuffer(bytearray(b"\xab" * (32 * max(cap, 1))), dtype=_abi.NODE_DTYPE)  # (writable)
    n = C.c_int(-1)
    rc = lib.oaz_tree_rebase_host(_abi.ptr(nodes), len(nodes), child, _abi.ptr(out), cap, C.byref(n))
    return rc, out, n.value


@pytest.mark.parametrize("sims,c_puct", CASES)
def test_c1_rebased_subtree_equals_fresh_search(lib, orc, sims, c_puct):
    checked = 0
    for r in usable_roots(orc, 20, seed=1300 + sims):
        r = r.reshape(1)
        _, _, nodes, _ = orc.search(orc.search_cfg(sims=sims, c_puct=c_puct), r)
        root = nodes[0]
        assert root["flags"] & 1
        for k in range(int(root["nch"])):
            ch = nodes[int(root["first"]) + k]
            pos, res = stepped(orc, r, unpack(ch["mv"]))
            if ch["N"] == 0 or ch["flags"] & 2 or res in (1, 2):
                continue
            rc, out, n = rebase_host(lib, nodes, k)
            assert rc == 0
            _, _, ref, _ = orc.search(orc.search_cfg(sims=int(ch["N"]), c_puct=c_puct), pos)
            assert n == len(ref)
            assert_trees_equal(out[:n], ref)
            assert not out[:n]["pad"].any()
            assert out[n:].tobytes() == b"\xab" * (32 * (len(out) - n))  # nothing past the subtree is written
            checked += 1
    assert checked >= 60


def test_c2_errors_write_nothing(lib, orc):
    r = usable_roots(orc, 1, seed=5)
    _, _, one, _ = orc.search(orc.search_cfg(sims=1, c_puct=2.0), r)  # one playout expands the root only
    _, _, nodes, _ = orc.search(orc.search_cfg(sims=12, c_puct=5.0), r)
    root = nodes[0]
    kids = nodes[int(root["first"]):int(root["first"]) + int(root["nch"])]
    unvisited = [k for k in range(len(kids)) if kids[k]["N"] == 0]
    visited = [k for k in range(len(kids)) if kids[k]["N"] >= 2 and kids[k]["flags"] == 1]
    assert unvisited and visited  # 12 playouts leave some of the root's children unvisited
    u = kids[unvisited[0]]
    assert (u["first"], u["nch"], u["flags"]) == (0, 0, 0)  # never expanded: the leaf-root case
    cases = [(one[:1], 0, None, _abi.ERR_ARG),                         # child 0 of a one-node tree
             (nodes, int(root["nch"]), None, _abi.ERR_ARG),            # a child out of range
             (nodes, -1, None, _abi.ERR_ARG),
             (nodes, unvisited[0], None, _abi.ERR_ARG),                # an unvisited child
             (nodes, visited[0], 1, _abi.ERR_CAPACITY)]                # cap too small
    for tree, child, cap, want in cases:
        rc, out, n = rebase_host(lib, tree, child, cap)
        assert rc == want, (child, cap, rc)
        assert n == -1 and out.tobytes() == b"\xab" * (32 * len(out))
        assert lib.oaz_last_error()


def test_c3_abi(lib):
    assert C.sizeof(_abi.oaz_config) == 120 and _abi.oaz_config.reuse_visits.offset == 116
    assert _abi.default_config().reuse_visits == 0
    assert lib.oaz_abi_version() == 5
    for name in ("oaz_search_advance", "oaz_search_resume", "oaz_reuse_stats_get", "oaz_tree_rebase_host"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_abi.oaz_reuse_stats) == 32
    # 0 < reuse_visits < sims: OAZ_ERR_ARG before a device is touched (with or without one)
    cfg = _abi.default_config()
    cfg.sims, cfg.reuse_visits, cfg.games = 64, 63, 4
    assert not lib.oaz_create(C.byref(cfg), 0)
    assert b"reuse_visits=63 < sims=64" in lib.oaz_last_error()
    cfg.reuse_visits = -1
    assert not lib.oaz_create(C.byref(cfg), 0)
    assert b"out of range" in lib.oaz_last_error()
    if _abi.device_count() == 0:  # a valid setting gets as far as the device check
        cfg.reuse_visits = 64
        assert not lib.oaz_create(C.byref(cfg), 0)
        assert b"no HIP device" in lib.oaz_last_error()


def test_c4_c_program_under_sanitizers(tmp_path):
    """tests/c/rebase_smoke.c with csrc/oaz_tree_rebase.cpp compiled host-only, both with
    -fsanitize=address,undefined: a stand-alone program (nothing is loaded into Python)."""
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++") or shutil.which("c++")
    if cc is None or cxx is None:
        pytest.skip("no C / C++ compiler")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-Wall", "-Werror"]
    obj, main, exe = tmp_path / "oaz_tree_rebase.o", tmp_path / "rebase_smoke.o", tmp_path / "rebase_smoke"
    subprocess.run([cxx, *san, "-std=c++17", "-DOAZ_REBASE_STANDALONE", "-c", str(CSRC / "oaz_tree_rebase.cpp"),
                    "-o", str(obj)], check=True)
    subprocess.run([cc, *san, f"-I{ROOT / 'include'}", "-c", str(ROOT / "tests/c/rebase_smoke.c"), "-o", str(main)],
                   check=True)
    subprocess.run([cxx, *san, str(main), str(obj), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK rebase" in r.stdout, r.stdout + r.stderr
