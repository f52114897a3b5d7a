"""What the search driver enqueues, pinned on the CPU: tests/c/engine_schedule.cpp links the real
csrc/oaz_engine.cpp (and oaz_pack.cpp), compiled host-only with the Makefile's flags, with recording fakes
of the HIP runtime calls and of the kernels' launchers (oaz_kernels.h). Every launch (kernel, stream, game
range, noise / policy / value pointers, budget pointers), every hipEventRecord / hipStreamWaitEvent /
hipStreamSynchronize and every asynchronous copy or fill of each scenario (the one-launch searches, the
per-step loop with parts, compaction, the root-noise ring, both budgets, self-play, failing launches) is one
line. Six scenarios (one of each path and kind) are printed in full; in the others the device calls between
two lines of the scenario itself are folded into "(N device calls, fnv1a H)", a digest of exactly those
lines, so every scenario is pinned alike and the file stays readable. The output is compared with
tests/golden/engine_schedule.txt line for line. When a digest differs, `engine_schedule --full` built from the
two versions of the engine prints every call, and `diff` shows what moved.

The golden file is this engine's own recorded output, taken before the driver was split into one function per
path. A change that is meant to alter the schedule re-records it and explains every differing line; a
refactor must reproduce it. To record (from the repository root):

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-result -DOAZ_AB=0 \\
        -x hip --cuda-host-only -no-hip-rt tests/c/engine_schedule.cpp \\
        onitama-alphazero_amd/csrc/oaz_engine.cpp onitama-alphazero_amd/csrc/oaz_pack.cpp -o engine_schedule
    ./engine_schedule > tests/golden/engine_schedule.txt
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "onitama-alphazero_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "engine_schedule.txt"
# csrc/Makefile's CXXFLAGS with AB=0, the engine's "-x hip", and host-only without the HIP runtime
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-result",
         "-DOAZ_AB=0", "-x", "hip", "--cuda-host-only", "-no-hip-rt"]


def _hipcc():
    cand = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    return cand if shutil.which(cand) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("engine_schedule") / "engine_schedule"
    srcs = [ROOT / "tests/c/engine_schedule.cpp", CSRC / "oaz_engine.cpp", CSRC / "oaz_pack.cpp"]
    subprocess.run([hipcc, *FLAGS, *map(str, srcs), "-o", str(exe)], check=True)
    return exe


def _run(exe, *args):
    return subprocess.run([str(exe), *args], capture_output=True, text=True, check=True).stdout.splitlines()


def _scenarios(lines):
    """{title: lines} of the "==== title" sections, in order."""
    out, cur = {}, None
    for ln in lines:
        if ln.startswith("==== "):
            cur = out.setdefault(ln[5:], [])
        else:
            assert cur is not None, "a line before the first scenario"
            cur.append(ln)
    return out


def test_schedule_equals_golden(recorder):
    recorded = _run(recorder)
    want = GOLDEN.read_text().splitlines()
    got_s, want_s = _scenarios(recorded), _scenarios(want)
    assert list(got_s) == list(want_s), "the scenarios and their order"
    for title, w in want_s.items():
        g = got_s[title]
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"scenario '{title}', line {i + 1}"
        assert len(g) == len(w), f"scenario '{title}': {len(g)} lines, golden {len(w)}"
    assert recorded == want


def test_scenarios_take_the_paths_they_are_named_for(recorder):
    """Every scenario's calls in full (--full): each ran the search it is meant to pin (so a re-recording
    that lost a path, e.g. by a changed threshold, fails here and not silently), and nothing but the device
    calls differs from the folded output."""
    recorded = _run(recorder, "--full")
    folded = [ln for ln in _run(recorder) if not ln.startswith("(")]
    kept = iter(recorded)
    assert all(any(ln == k for k in kept) for ln in folded), "the folded output's own lines, in order, are in the full one"
    s = _scenarios(recorded)

    def launches(title, kernel):
        return [ln for ln in s[title] if ln.startswith("#") and ln.split()[1] == kernel]

    assert len(launches("1 lat", "search_lat")) == 1 and not launches("1 lat", "expand_backup")
    assert len(launches("2 grp, one chunk", "search_grp")) == 1
    assert len(launches("3 grp, three chunks, 128 games", "search_grp")) == 3
    assert len(launches("3 grp, three chunks, 128 games", "root_noise")) == 3
    assert not launches("3 129 games: the per-step loop", "search_grp")
    assert len(launches("3 129 games: the per-step loop", "backup_select")) == 1099
    for title, parts in (("5 steps, NN, 2047 games (1 part)", 1), ("5 steps, NN, 2048 games (2 parts)", 2),
                         ("5 steps, NN, 8200 games, 4 parts (3 buckets)", 4)):
        assert [ln for ln in s[title] if ln.startswith("kernel_times") and ln.endswith(f" parts={parts}")]
    # the 8200 games' parts (2050 each) own 1 + 1 + 1 + 1 bucket counters: consecutive 4-byte offsets
    assert [ln.split("bcnt=")[1].split()[0].split("+")[1] for ln in launches(
        "5 steps, NN, 8200 games, 4 parts (3 buckets)", "select")] == ["0", "4", "8", "12"]
    assert not launches("6 compact 2, 1535 games", "eval_compact") and launches("6 compact 2, 1536 games", "eval_compact")
    assert "last_sims rc=0 sims=18" in s["7 steps, small, budget 1e9"]
    assert "last_sims rc=0 sims=1" in s["7 steps, small, budget 1 ns"]
    for title in s:
        if title.startswith("10 "):
            assert "search rc=-3 error=launch() failed: fake launch failure" in s[title]
            assert "destroyed last_error=launch() failed: fake launch failure" in s[title]
            i = next(k for k, ln in enumerate(s[title]) if ln.endswith("-> FAILS"))
            assert s[title][i + 1:i + 7] == ["record e2 on s3", "wait s1 for e2", "record e3 on s4", "wait s1 for e3",
                                             "record e4 on s5", "wait s1 for e4"], "the parts' streams are joined"
    assert not [ln for ln in recorded if "LEAKED" in ln or "!dead" in ln]
