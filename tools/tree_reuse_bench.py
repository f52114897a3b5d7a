#!/usr/bin/env python3
"""Self-play with tree reuse (oaz_config.reuse_visits) beside self-play without, on one GPU. Measurement tool;
bench.py is the flagship's and is not touched.

The flagship's engine (3-block network, random-init weights seed 0, fp16x3 split, 400 simulations, root noise,
fixed deck, staggered starts, compact 0, automatic parts) at 4 096 games (C2) and 65 536 games (C3), with
reuse_visits 0, 800 and 1200. Every configuration runs in a child process of its own under `timeout` (an engine
of 65 536 trees of 1 + 40 * 1200 nodes holds 100 GB; nothing of it should outlive its measurement), one at a
time; the first child without exit status 0 and a result ends the whole run (tools/ab.py).

Per configuration: `--warmup` plies (staggered starts over, trees at their steady-state sizes), then `--reps`
timed windows of `--plies` plies each, the host's monotonic clock around selfplay_step + sync. Reported: plies/s
per window, their median, minimum and maximum (the spread); over the timed windows the mean playouts per
search tree-reuse saved (visits_kept / (trees_kept + trees_fresh)), the share of searches that began on a kept
tree, the mean kept subtree (nodes), the mean tree when a search ends, the mean select depth, the largest tree, and the device memory of the trees
from their shape (games x (1 + 40 x R) nodes of 32 B).

`--parent DIR`: a checkout of the parent commit, built; the reuse_visits = 0 configuration is then also measured
with DIR's package and library, alternating with this tree's (this tree, parent, this tree, ...), and both are
recorded: with reuse off the engine must run as the parent does.

`--trace`: in further runs of their own, the reuse_visits > 0 configurations of the largest size under
`rocprofv3 --kernel-trace --stats` (fewer plies), for the rebase kernel's share of the kernel time.

usage: python tools/tree_reuse_bench.py [--out profiles/tree_reuse_<date>.json] [--sizes 4096,65536]
                                        [--reuse 0,800,1200] [--sims 400] [--warmup 14] [--plies 4] [--reps 5]
                                        [--parent DIR] [--trace | --trace-only]"""
from __future__ import annotations

import argparse
import csv
import datetime
import json
import shutil
import statistics
import sys
import time
from pathlib import Path

import ab

ROOT = Path(__file__).resolve().parents[1]


def child(args) -> None:
    """One configuration, in this process: prints one JSON line."""
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    stagger = min(12, args.warmup)
    kw = dict(games=args.games, sims=args.sims, blocks=3, c_puct=5.0, train_noise=1, max_plies=150,
              evaluator=_abi.EVAL_NN, precision=_abi.FP32_SPLIT16, fixed_deck=1, deck=[0, 1, 2, 3, 4], seed=20260101,
              sample_capacity=args.games * 8, stagger=stagger, compact=0, parts=0)
    if args.reuse_visits:  # (the parent's config has no such field)
        kw["reuse_visits"] = args.reuse_visits
    with Engine(**kw) as e:
        e.load_weights(random_weights(0, 3))
        e.selfplay_reset()
        for _ in range(args.warmup):
            e.selfplay_step(1)
        e.sync()
        st0 = e.selfplay_stats()
        rs0 = e.reuse_stats() if args.reuse_visits else None
        rates = []
        for _ in range(args.reps):
            e.samples_fetch(args.games * 8)  # (the buffer never fills: dropped samples would not slow a ply, but still)
            e.sync()
            t0 = time.perf_counter()
            e.selfplay_step(args.plies)
            e.sync()
            rates.append(args.games * args.plies / (time.perf_counter() - t0))
        st1 = e.selfplay_stats()
        out = {"games": args.games, "sims": args.sims, "reuse_visits": args.reuse_visits, "plies_per_window": args.plies,
               "plies_per_s": [round(r, 1) for r in rates], "median_plies_per_s": statistics.median(rates),
               "min_plies_per_s": min(rates), "max_plies_per_s": max(rates),
               "moves": int(st1.moves - st0.moves),
               "playouts_run_per_search": (st1.search.sims - st0.search.sims) / max(1, st1.moves - st0.moves),
               "mean_select_depth": (st1.search.depth_sum - st0.search.depth_sum) / max(1, st1.search.sims - st0.search.sims),
               "max_tree_nodes": int(st1.search.max_nodes),
               # a search's tree when it ends: the root or the kept subtree it began on + the children it added
               "mean_tree_nodes": 1 + (st1.search.children - st0.search.children) / max(1, st1.moves - st0.moves),
               "tree_bytes": args.games * (1 + 40 * (args.reuse_visits or args.sims)) * 32}
        if rs0 is not None:
            rs1 = e.reuse_stats()
            kept, fresh = rs1.trees_kept - rs0.trees_kept, rs1.trees_fresh - rs0.trees_fresh
            out["mean_tree_nodes"] = ((st1.search.children - st0.search.children) + fresh +
                                      (rs1.nodes_kept - rs0.nodes_kept)) / max(1, kept + fresh)
            out.update(trees_kept=int(kept), trees_fresh=int(fresh),
                       visits_kept_per_search=(rs1.visits_kept - rs0.visits_kept) / max(1, kept + fresh),
                       kept_share=kept / max(1, kept + fresh),
                       mean_kept_subtree_nodes=(rs1.nodes_kept - rs0.nodes_kept) / max(1, kept))
    print("RESULT " + json.dumps(out), flush=True)


def child_cmd(args, games, reuse, pkg=None, trace_dir=None) -> list:
    """The command of one configuration's child process; traced, the program goes after `rocprofv3 ... --`."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--games", str(games), "--reuse-visits", str(reuse),
           "--sims", str(args.sims), "--warmup", str(args.warmup), "--plies", str(args.plies if not trace_dir else 2),
           "--reps", str(args.reps if not trace_dir else 1)]
    if pkg:
        cmd += ["--pkg", str(pkg)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", str(trace_dir), "--"] + cmd
    return cmd


def rebase_share(trace_dir: Path):
    """The rebase kernel's share of the traced kernel time, from rocprofv3's kernel statistics."""
    for f in sorted(trace_dir.rglob("*kernel_stats.csv")):
        rows = list(csv.DictReader(f.open()))
        total = sum(float(r.get("TotalDurationNs", 0) or 0) for r in rows)
        mine = [r for r in rows if "k_selfplay_rebase" in r.get("Name", "")]
        if mine and total > 0:
            ns = sum(float(r["TotalDurationNs"]) for r in mine)
            return {"rebase_ns": ns, "all_kernels_ns": total, "share_of_kernel_time": ns / total,
                    "calls": sum(int(r.get("Calls", 0) or 0) for r in mine),
                    "mean_ns_per_call": ns / max(1, sum(int(r.get("Calls", 0) or 0) for r in mine))}
    return None


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reuse", default="0,800,1200")
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-only", action="store_true", help="only the --trace runs, added to an existing --out file")
    ap.add_argument("--trace-dir", default=None, help="where the rocprofv3 output goes (default: beside --out)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--reuse-visits", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"tree_reuse_{date}.json")
    sizes = [int(x) for x in args.sizes.split(",")]
    reuse = [int(x) for x in args.reuse.split(",")]
    doc = {"tool": "tools/tree_reuse_bench.py", "date": date, "sims": args.sims, "warmup_plies": args.warmup,
           "method": "per configuration a child process; warm-up plies, then `reps` windows of `plies_per_window` plies, "
                     "host clock around selfplay_step + sync; plies/s = games x plies / window",
           "runs": [], "parent_runs": [], "traces": []}
    if args.trace_only:
        if not out.exists():
            raise SystemExit(f"--trace-only adds to an existing file, and {out} does not exist")
        doc = json.loads(out.read_text())
        doc["traces"] = []
    run = ab.Run(out, doc)
    for games in ([] if args.trace_only else sizes):
        for R in reuse:
            sides, both = [(None, "runs")], R == 0 and args.parent
            if both:  # this tree and the parent, alternating, twice each
                sides.append((Path(args.parent) / "onitama-alphazero_amd", "parent_runs"))
            for pkg, key in ab.schedule(sides, 2 if both else 1):
                what = f"games {games} reuse_visits {R} {'parent' if pkg else 'this tree'}"
                res = run.child(what, child_cmd(args, games, R, pkg=pkg), 900)[-1]
                print(f"{what}: {round(res['median_plies_per_s'], 1)} plies/s", flush=True)
                doc[key].append(res)
                run.save()
    if args.trace or args.trace_only:
        if not shutil.which("rocprofv3"):
            raise SystemExit("--trace needs rocprofv3")
        for R in [r for r in reuse if r > 0]:
            td = Path(args.trace_dir or out.parent / f"tree_reuse_trace_{date}") / f"R{R}"
            run.child(f"trace games {sizes[-1]} reuse_visits {R}", child_cmd(args, sizes[-1], R, trace_dir=td), 900)
            share = rebase_share(td)
            doc["traces"].append({"games": sizes[-1], "reuse_visits": R, "exit": 0, "kernel_trace": share,
                                  "note": "rocprofv3 --kernel-trace --stats, a run of its own: warm-up plies + 2 plies"})
            print(f"trace games {sizes[-1]} reuse_visits {R}: {share}", flush=True)
            run.save()
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
