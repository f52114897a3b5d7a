#!/usr/bin/env python3
"""Same-box A/B harness: one child at a time under `timeout`, sides alternating, and nothing more started after
the first child that is not good. A module (the bench tools in tools/ import it) and a command.

A child is good only with exit status 0 and at least one record. Its records are the stdout lines `RESULT <json>`;
if there is none, the stdout lines that are JSON objects (bench.py prints one last, tools/tree_noise_probe.py two);
if there is none, the whole of stdout as one object (tools/nn_ab.py, tools/search_latency.py). Anything else ends
the run: the document is saved, the child's last output goes to stderr, the status is named, and the process exits
non-zero. Nothing is retried.

usage: python tools/ab.py [--rounds N] [--limit SECONDS] [--tests "PYTEST ARGS"] [--show KEY[,KEY...]] [--out FILE]
                          --side NAME[:VAR=VALUE[,VAR=VALUE...]] [--side ...] -- COMMAND...

A side is a name and environment settings; a side without settings runs the environment as it is. The command runs
from this checkout's root, so OAZ_LIB may be given relative to it. `--tests` first runs the GPU tests named under
each side's environment. `--show` keys are dotted paths into a record. L below is onitama-alphazero_amd/onitama_az.

Recipes (SHORT = --no-cpu-baseline --no-exact --no-pmc --no-allgather; LIBS = --side prev:OAZ_LIB=L/libonitama_az_prev.so
--side tree:OAZ_LIB=L/libonitama_az.so; SHOW = --show value,ms_per_step,kernel_ms_per_step.search_grp):
  C3, two libraries:   ab.py --rounds 2 LIBS SHOW -- python bench.py --steps 4 --warmup 14 SHORT
  C2 / C5:             ab.py LIBS SHOW -- python bench.py --config c2 SHORT      (c5: --config c5 --steps 3 --warmup 6 SHORT)
  training step:       ab.py --limit 200 --tests tests/test_train.py LIBS --show ms_per_step -- python bench.py --mode train --steps 200 --warmup 20 --no-cpu-baseline
  pure MCTS:           ab.py --rounds 2 --tests tests/test_pure_mcts.py LIBS --show value,ms_per_step -- python bench.py --mode pure_mcts --steps 2 --warmup 1 --no-cpu-baseline --no-pmc
  Agent latency:       ab.py --rounds 2 --tests 'tests/test_gpu_agent.py tests/test_gpu.py -k "agent or one_launch or time_budget"' --side prev:OAZ_LIB=L/libonitama_az_prev.so,OAZ_LAT_G=1,OAZ_LAT_BUDGETS=0 --side tree:OAZ_LIB=L/libonitama_az.so,OAZ_LAT_G=1,OAZ_LAT_BUDGETS=0 --show G1.ms_median,G1.ms_min -- python tools/search_latency.py 400 10
  tree kernel probe:   ab.py --limit 200 LIBS --show noise,ms_per_ply,backup_select_us,noise_ms_per_ply -- python tools/tree_noise_probe.py
  NN kernel, fp16x3:   ab.py --rounds 8 --limit 120 LIBS --show 3-fp32h3-v0.median_ms -- python tools/nn_ab.py --blocks 3 --precision fp32h3 --rounds 2
  NN kernel, bf16:     ab.py --rounds 8 --limit 120 LIBS --show 6-bf16.median_ms -- python tools/nn_ab.py --blocks 6 --precision bf16 --rounds 2
  A/B build's knobs:   ab.py --side seg0:OAZ_LIB=L/libonitama_az_ab.so,OAZ_TREE_SEG=0 --side seg1:OAZ_LIB=L/libonitama_az_ab.so,OAZ_TREE_SEG=1 SHOW -- python bench.py --config c2 SHORT"""
from __future__ import annotations

import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MEANING = {124: "time limit", 137: "killed", 134: "abort", 139: "segmentation fault"}
PYTEST = ["-x", "-q", "-m", "gpu", "--timeout", "250", "--timeout-method", "thread"]
Child = namedtuple("Child", "status records tail")


def records(stdout: str) -> list:
    """A child's records: `RESULT <json>` lines, else the lines that are JSON objects, else all of stdout as one."""
    def objects(texts):
        found = []
        for text in texts:
            try:
                found.append(json.loads(text))
            except ValueError:
                pass
        return [obj for obj in found if isinstance(obj, dict)]

    lines = stdout.splitlines()
    return objects(ln[7:] for ln in lines if ln.startswith("RESULT ")) or objects(lines) or objects([stdout])


def one_child(cmd, limit, env=None, cwd=None) -> Child:
    """`cmd` under `timeout -k 10 limit`, `env` laid over the environment: (exit status, records, last output)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + [str(c) for c in cmd], capture_output=True, text=True,
                       env=dict(os.environ, **env) if env else None, cwd=cwd)
    return Child(p.returncode, records(p.stdout), p.stdout[-2000:] + p.stderr[-4000:])


def schedule(sides, rounds) -> list:
    """The sides in the order given, `rounds` times: A B A B ..."""
    return list(sides) * rounds


def spread_verdict(mine, other, higher_is_better) -> dict:
    """The acceptance rule: this tree's slower run may be behind the other side's slower run by no more than the
    other side's runs differ from each other."""
    a, b = sorted(mine), sorted(other)
    behind = b[0] - a[0] if higher_is_better else a[-1] - b[-1]
    return {"mine": a, "other": b, "other_spread": b[-1] - b[0], "behind_by": behind, "accepted": behind <= b[-1] - b[0]}


class Run:
    """A result document, written to `out` after every child, and the stop rule."""

    def __init__(self, out, doc):
        self.out, self.doc = Path(out) if out else None, doc

    def save(self) -> None:
        if self.out:
            self.out.parent.mkdir(parents=True, exist_ok=True)
            self.out.write_text(json.dumps(self.doc, indent=1) + "\n")

    def child(self, what, cmd, limit, env=None, cwd=None, needs_record=True) -> list:
        """The records of a good child; after any other, saves the document and ends the process."""
        c = one_child(cmd, limit, env, cwd)
        if c.status == 0 and (c.records or not needs_record):
            return c.records
        self.save()
        sys.stderr.write(c.tail)
        meaning = MEANING.get(c.status, "failed" if c.status else "no record")
        raise SystemExit(f"{what}: the child ended with status {c.status} ({meaning}) and {len(c.records)} record(s): "
                         "nothing more is started")


def lookup(record, path):
    for k in path.split("."):
        record = record.get(k) if isinstance(record, dict) else None
    return record


def parse_side(text):
    name, _, settings = text.partition(":")
    return name, dict(s.split("=", 1) for s in settings.split(",") if s)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    ap.add_argument("--tests", default=None, help="pytest arguments: the GPU tests each side passes first")
    ap.add_argument("--show", default="", help="dotted paths into a record, comma-separated")
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", action="append", required=True, type=parse_side)
    ap.add_argument("command", nargs="+")
    args = ap.parse_args()
    keys = [k for k in args.show.split(",") if k]
    sides = dict(args.side)
    run = Run(args.out, {"tool": "tools/ab.py", "command": args.command, "rounds": args.rounds, "limit": args.limit,
                         "sides": sides, "tests": [], "order": [], "runs": {name: [] for name in sides}})
    for name in (sides if args.tests else []):
        run.child(f"{name} tests", [sys.executable, "-m", "pytest"] + shlex.split(args.tests) + PYTEST, 300,
                  sides[name], ROOT, needs_record=False)
        run.doc["tests"].append(name)
        print(f"{name} tests: passed", flush=True)
        run.save()
    seen = {}
    for k, name in enumerate(schedule(sides, args.rounds)):
        recs = run.child(f"{name} round {k // len(sides) + 1}", args.command, args.limit, sides[name], ROOT)
        run.doc["order"].append(name)
        run.doc["runs"][name].append(recs)
        run.save()
        for i, rec in enumerate(recs):
            shown = {key: lookup(rec, key) for key in keys} if keys else rec
            print(f"{name} round {k // len(sides) + 1}: {json.dumps(shown)}", flush=True)
            for key in keys:
                if isinstance(shown[key], (int, float)):
                    seen.setdefault((name, i, key), []).append(shown[key])
    for (name, i, key), v in seen.items():
        print(f"{name} record {i} {key}: n {len(v)} mean {statistics.mean(v):.6g} median {statistics.median(v):.6g} "
              f"min {min(v):.6g} max {max(v):.6g}")


if __name__ == "__main__":
    main()
