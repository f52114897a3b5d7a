"""tools/ab.py, the A/B harness: schedule, environment overlay, record parsing, the stop rule and the acceptance
rule, and the four bench tools that run their children through it. No GPU and no library: the children are tiny
`python -c` programs."""
import importlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import ab  # noqa: E402

# One child for every case: logs that it started, then does what AB_MODE says (a side's setting).
CHILD = """
import json, os, sys, time
log, mode = os.environ["AB_LOG"], os.environ.get("AB_MODE", "ok")
n = len(open(log).read().split()) if os.path.exists(log) else 0
open(log, "a").write(mode + "\\n")
if mode == "segv":
    os._exit(139)
if mode == "sleep":
    time.sleep(30)
if mode != "silent":
    print(json.dumps({"n": n, "mode": mode, "var": os.environ.get("AB_VAR"), "deep": {"er": 2.5}}), flush=True)
if mode == "exit1":
    os._exit(1)
"""


def run_ab(tmp_path, *args, command=(sys.executable, "-c", CHILD)):
    """tools/ab.py as a command: (process, started children's modes in order, the --out document or None)."""
    log, out = tmp_path / "log", tmp_path / "out.json"
    env = {k: v for k, v in os.environ.items() if k not in ("AB_MODE", "AB_VAR")}
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "ab.py"), "--out", str(out), *args, "--", *command],
                       capture_output=True, text=True, env=dict(env, AB_LOG=str(log)), timeout=60)
    return p, log.read_text().split() if log.exists() else [], json.loads(out.read_text()) if out.exists() else None


def test_schedule_alternates_and_files_records_by_side(tmp_path):
    assert ab.schedule(["A", "B"], 3) == ["A", "B", "A", "B", "A", "B"]
    p, started, doc = run_ab(tmp_path, "--rounds", "3", "--side", "a:AB_MODE=ok", "--side", "b:AB_MODE=other",
                             "--show", "n,deep.er")
    assert p.returncode == 0, p.stderr
    assert started == ["ok", "other"] * 3
    assert doc["order"] == ["a", "b"] * 3
    assert [[r["n"] for r in recs] for recs in doc["runs"]["a"]] == [[0], [2], [4]]
    assert [[r["n"] for r in recs] for recs in doc["runs"]["b"]] == [[1], [3], [5]]
    lines = p.stdout.splitlines()
    assert lines[:2] == ['a round 1: {"n": 0, "deep.er": 2.5}', 'b round 1: {"n": 1, "deep.er": 2.5}']
    assert "a record 0 n: n 3 mean 2 median 2 min 0 max 4" in lines
    assert "b record 0 deep.er: n 3 mean 2.5 median 2.5 min 2.5 max 2.5" in lines


def test_a_sides_settings_reach_its_child_only(tmp_path):
    p, _, doc = run_ab(tmp_path, "--rounds", "2", "--side", "a:AB_VAR=x=1,AB_MODE=ok", "--side", "b")
    assert p.returncode == 0, p.stderr
    assert [recs[0]["var"] for recs in doc["runs"]["a"]] == ["x=1", "x=1"]
    assert [recs[0]["var"] for recs in doc["runs"]["b"]] == [None, None]
    assert doc["sides"] == {"a": {"AB_VAR": "x=1", "AB_MODE": "ok"}, "b": {}}


def test_record_parsing():
    assert ab.records('noise\nRESULT {"a": 1}\nmore\nRESULT {"a": 2}\n') == [{"a": 1}, {"a": 2}]
    assert ab.records('warming up\n{"lib": "x", "noise": 1}\n[1, 2]\n3\n{"lib": "x", "noise": 0}\n') == \
        [{"lib": "x", "noise": 1}, {"lib": "x", "noise": 0}]
    assert ab.records(json.dumps({"G1": {"ms_median": 1.5}, "G16": {"ms_median": 2.5}}, indent=1) + "\n") == \
        [{"G1": {"ms_median": 1.5}, "G16": {"ms_median": 2.5}}]
    assert ab.records('{"bare": 1}\nRESULT {"a": 1}\n{"bare": 2}\n') == [{"a": 1}]
    assert ab.records("") == [] and ab.records("no record here\n") == [] and ab.records("[1, 2]\n") == []


def test_one_child_returns_status_and_records():
    c = ab.one_child([sys.executable, "-c", "import os; print('RESULT {\"v\": \"' + os.environ['AB_VAR'] + '\"}')"],
                     20, env={"AB_VAR": "7"})
    assert (c.status, c.records) == (0, [{"v": "7"}])
    c = ab.one_child([sys.executable, "-c", "import sys; print('to stdout'); sys.exit('to stderr')"], 20)
    assert c.status == 1 and c.records == [] and "to stdout" in c.tail and "to stderr" in c.tail


def test_a_fault_ends_the_run(tmp_path):
    p, started, doc = run_ab(tmp_path, "--rounds", "2", "--side", "a", "--side", "b:AB_MODE=segv")
    assert p.returncode != 0
    assert started == ["ok", "segv"]  # the third child of the schedule would have logged its start
    assert [[r["n"] for r in recs] for recs in doc["runs"]["a"]] == [[0]] and doc["runs"]["b"] == []
    assert "status 139 (segmentation fault)" in p.stderr and "nothing more is started" in p.stderr


def test_the_time_limit_ends_the_run(tmp_path):
    t0 = time.monotonic()
    p, started, doc = run_ab(tmp_path, "--limit", "1", "--side", "a:AB_MODE=sleep", "--side", "b")
    assert time.monotonic() - t0 < 10
    assert p.returncode != 0 and started == ["sleep"]
    assert doc["runs"] == {"a": [], "b": []}
    assert "status 124 (time limit)" in p.stderr


@pytest.mark.parametrize("mode, said", [("exit1", "status 1 (failed) and 1 record(s)"),
                                        ("silent", "status 0 (no record) and 0 record(s)")])
def test_a_result_with_exit_1_and_exit_0_without_a_record_end_the_run(tmp_path, mode, said):
    p, started, doc = run_ab(tmp_path, "--side", "a", "--side", f"b:AB_MODE={mode}")
    assert p.returncode != 0 and started == ["ok", mode]
    assert len(doc["runs"]["a"]) == 1 and doc["runs"]["b"] == []
    assert said in p.stderr


def test_failing_tests_start_no_measurement(tmp_path):
    p, started, doc = run_ab(tmp_path, "--tests", "tests/no_such_test_file.py", "--side", "a", "--side", "b")
    assert p.returncode != 0 and started == []
    assert doc["tests"] == [] and doc["order"] == []
    assert "a tests: the child ended with status 4" in p.stderr


def test_spread_verdict_reproduces_the_recorded_verdicts():
    # profiles/temperature_2026-10-20.json, off_against_parent: plies/s, higher is better
    for mine, parent, spread, behind, accepted in (
            ([118204.10624719363, 118934.59861733518], [117403.25799131728, 118406.2697719372],
             1003.0117806199123, -800.8482558763499, True),
            ([131381.51474524575, 132706.36668727337], [132174.49435517908, 132694.60287051182],
             520.108515332744, 792.9796099333325, False)):
        v = ab.spread_verdict(reversed(mine), reversed(parent), higher_is_better=True)
        assert v == {"mine": mine, "other": parent, "other_spread": spread, "behind_by": behind, "accepted": accepted}
    # profiles/reflect_2026-10-21.json, absent_against_parent: ms per step, lower is better
    v = ab.spread_verdict([0.7620876259579745, 0.751893311985441], [0.7533191665061167, 0.7555632387834521],
                          higher_is_better=False)
    assert v == {"mine": [0.751893311985441, 0.7620876259579745], "other": [0.7533191665061167, 0.7555632387834521],
                 "other_spread": 0.0022440722773353627, "behind_by": 0.006524387174522417, "accepted": False}


def test_spread_verdict_accepts_equality_and_nothing_past_it():
    # the other side's runs differ by 2: this tree's slower run may be 2 behind, and not 3
    assert ab.spread_verdict([98, 105], [100, 102], higher_is_better=True)["accepted"] is True
    assert ab.spread_verdict([97, 105], [100, 102], higher_is_better=True)["accepted"] is False
    assert ab.spread_verdict([90, 104], [100, 102], higher_is_better=False)["accepted"] is True
    assert ab.spread_verdict([90, 105], [100, 102], higher_is_better=False)["accepted"] is False
    assert ab.spread_verdict([98, 105], [100, 102], higher_is_better=True)["behind_by"] == 2
    assert ab.spread_verdict([90, 105], [100, 102], higher_is_better=False)["behind_by"] == 3


BENCH_TOOLS = ["tree_reuse_bench", "temperature_bench", "leaf_batch_bench", "reflect_bench"]


@pytest.mark.parametrize("tool", BENCH_TOOLS)
def test_bench_tools_import_and_parse_help(tool, monkeypatch, capsys):
    mod = importlib.import_module(tool)
    monkeypatch.setattr(sys, "argv", [f"tools/{tool}.py", "--help"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 0 and "--out" in capsys.readouterr().out
    for gone in ("FAULTS", "run_child", "off_verdict", "absent_verdict", "subprocess"):
        assert not hasattr(mod, gone)


def test_a_bench_tool_stops_at_a_failing_child(tmp_path, monkeypatch):
    """temperature_bench.py's own main, its child command pointed at a stub: the first child is good, the second
    prints its result and exits 1, and T = 0 would have been followed by T = 8."""
    tool = importlib.import_module("temperature_bench")
    stub = ("import os, sys; first = not os.path.exists(sys.argv[1]); open(sys.argv[1], 'a').write('x'); "
            "print('RESULT {\"median_plies_per_s\": 1.0}', flush=True); os._exit(0 if first else 1)")
    monkeypatch.setattr(tool, "child_cmd", lambda *a, **k: [sys.executable, "-c", stub, str(tmp_path / "started")])
    out = tmp_path / "temperature.json"
    monkeypatch.setattr(sys, "argv", ["tools/temperature_bench.py", "--out", str(out), "--sizes", "64", "--temps", "0,8"])
    with pytest.raises(SystemExit) as e:
        tool.main()
    assert e.value.code not in (0, None) and "status 1" in str(e.value.code)
    assert (tmp_path / "started").read_text() == "xx"
    doc = json.loads(out.read_text())
    assert doc["runs"] == [{"median_plies_per_s": 1.0}] and doc["parent_runs"] == [] and doc["diversity"] == []
    assert set(doc) == {"tool", "date", "sims", "warmup_plies", "method", "runs", "parent_runs", "off_against_parent",
                        "diversity"}
