#!/usr/bin/env python3
"""Self-play with temperature (oaz_config.temperature_plies) beside self-play without, on one GPU: what the draws
cost in plies/s and what they buy in different games. Measurement tool; bench.py is the flagship's and is not
touched.

The flagship's engine (3-block network, random-init weights seed 0, fp16x3 split, 400 simulations, root noise,
fixed deck, compact 0, automatic parts). Every configuration runs in a child process of its own under `timeout`,
one at a time; the first child without exit status 0 and a result ends the whole run (tools/ab.py).

Throughput (`--sizes`, default 4 096 and 65 536 games; T in `--temps`, default 0, 8, 30): staggered starts,
`--warmup` plies, then `--reps` timed windows of `--plies` plies each, the host's monotonic clock around
selfplay_step + sync, as tools/tree_reuse_bench.py. Reported: plies/s per window, their median, minimum and
maximum, and the share of the windows' plies that drew their move. `--parent DIR`: a checkout of the parent
commit, built; T = 0 is then also measured with DIR's package and library, alternating with this tree's (this
tree, parent, this tree, parent), and both are recorded. T = 0 is accepted when this tree's slower run is no
slower than the parent's slower run by more than the parent's two runs differ from each other.

Diversity (`--diversity-games`, default 4 096, T in `--temps`): the games 0 .. n-1 played to their end
(selfplay_run, every slot one game) and their records fetched. A game's records are consecutive and begin with
the start position, which with a fixed deck is the same for all. Reported: the number of distinct games (by the
sequence of recorded positions, which is the sequence of moves but the last), the share of distinct positions
among the samples, the mean plies per game, the draws and the share of draws whose child is not the most visited.

usage: python tools/temperature_bench.py [--out profiles/temperature_<date>.json] [--sizes 4096,65536]
                                         [--temps 0,8,30] [--sims 400] [--warmup 14] [--plies 4] [--reps 5]
                                         [--parent DIR] [--diversity-games 4096] [--no-throughput]"""
from __future__ import annotations

import argparse
import datetime
import json
import statistics
import sys
import time
from pathlib import Path

import ab

ROOT = Path(__file__).resolve().parents[1]


def engine_kw(_abi, args, **more):
    kw = dict(games=args.games, sims=args.sims, blocks=3, c_puct=5.0, train_noise=1, max_plies=150,
              evaluator=_abi.EVAL_NN, precision=_abi.FP32_SPLIT16, fixed_deck=1, deck=[0, 1, 2, 3, 4], seed=20260101,
              compact=0, parts=0, **more)
    if args.temperature:  # (the parent's config has no such field)
        kw["temperature_plies"] = args.temperature
    return kw


def child_throughput(args) -> None:
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    with Engine(**engine_kw(_abi, args, sample_capacity=args.games * 8, stagger=min(12, args.warmup))) as e:
        e.load_weights(random_weights(0, 3))
        e.selfplay_reset()
        for _ in range(args.warmup):
            e.selfplay_step(1)
        e.sync()
        st0 = e.selfplay_stats()
        ts0 = e.temperature_stats() if args.temperature else (0, 0)
        rates = []
        for _ in range(args.reps):
            e.samples_fetch(args.games * 8)  # (the buffer never fills)
            e.sync()
            t0 = time.perf_counter()
            e.selfplay_step(args.plies)
            e.sync()
            rates.append(args.games * args.plies / (time.perf_counter() - t0))
        st1 = e.selfplay_stats()
        ts1 = e.temperature_stats() if args.temperature else (0, 0)
        moves = int(st1.moves - st0.moves)
        out = {"games": args.games, "sims": args.sims, "temperature_plies": args.temperature,
               "plies_per_window": args.plies, "plies_per_s": [round(r, 1) for r in rates],
               "median_plies_per_s": statistics.median(rates), "min_plies_per_s": min(rates),
               "max_plies_per_s": max(rates), "moves": moves, "games_finished_in_windows":
               int(st1.games_finished - st0.games_finished), "draws": ts1[0] - ts0[0],
               "drawn_share_of_plies": (ts1[0] - ts0[0]) / max(1, moves),
               "mean_tree_nodes": 1 + (st1.search.children - st0.search.children) / max(1, moves)}
    print("RESULT " + json.dumps(out), flush=True)


def child_diversity(args) -> None:
    import numpy as np

    sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    n = args.games
    with Engine(**engine_kw(_abi, args, sample_capacity=n * 152)) as e:
        e.load_weights(random_weights(0, 3))
        t0 = time.perf_counter()
        got, st = e.selfplay_run(n, cap=n * 152)
        secs = time.perf_counter() - t0
        draws, differ = e.temperature_stats()
    states = np.ascontiguousarray(got["state"])
    rows = states.view(np.dtype((np.void, states.dtype.itemsize))).reshape(-1)
    starts = np.flatnonzero(rows == rows[0])  # the start position (fixed deck): a game's first record
    games = {rows[a:b].tobytes() for a, b in zip(starts, list(starts[1:]) + [len(rows)])}
    out = {"games": n, "sims": args.sims, "temperature_plies": args.temperature, "games_finished": int(st.games_finished),
           "games_by_start_position": int(len(starts)), "distinct_games": len(games), "samples": int(len(rows)),
           "distinct_positions": int(len(np.unique(rows))), "distinct_position_share": len(np.unique(rows)) / max(1, len(rows)),
           "mean_plies_per_game": len(rows) / max(1, int(st.games_finished)), "games_cut": int(st.games_cut),
           "red_wins": int(st.red_wins), "blue_wins": int(st.blue_wins), "draws": draws, "draws_not_most_visited": differ,
           "share_of_draws_not_most_visited": differ / max(1, draws), "samples_dropped": int(st.samples_dropped),
           "seconds": round(secs, 2)}
    print("RESULT " + json.dumps(out), flush=True)


def child_cmd(args, mode, games, T, pkg=None) -> list:
    """The command of one configuration's child process."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", mode, "--games", str(games), "--temperature", str(T),
           "--sims", str(args.sims), "--warmup", str(args.warmup), "--plies", str(args.plies), "--reps", str(args.reps)]
    return cmd + (["--pkg", str(pkg)] if pkg else [])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--temps", default="0,8,30")
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--diversity-games", type=int, default=4096, help="0: no diversity runs")
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--child", default=None, choices=["throughput", "diversity"], help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--temperature", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_throughput(args) if args.child == "throughput" else child_diversity(args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"temperature_{date}.json")
    temps = [int(x) for x in args.temps.split(",")]
    doc = {"tool": "tools/temperature_bench.py", "date": date, "sims": args.sims, "warmup_plies": args.warmup,
           "method": "per configuration a child process. throughput: staggered starts, warm-up plies, then `reps` windows "
                     "of `plies_per_window` plies, host clock around selfplay_step + sync; plies/s = games x plies / "
                     "window. diversity: selfplay_run of games 0 .. n-1 on n slots, all records fetched",
           "runs": [], "parent_runs": [], "off_against_parent": {}, "diversity": []}

    run = ab.Run(out, doc)

    def one(mode, games, T, pkg, key):
        what = f"{mode} games {games} T {T} {'parent' if pkg else 'this tree'}"
        res = run.child(what, child_cmd(args, mode, games, T, pkg=pkg), 900)[-1]
        print(f"{what}: {round(res['median_plies_per_s'], 1) if mode == 'throughput' else res['distinct_games']}", flush=True)
        doc[key].append(res)
        run.save()

    for games in ([] if args.no_throughput else [int(x) for x in args.sizes.split(",")]):
        for T in temps:
            sides = [(None, "runs")]
            if T == 0 and args.parent:  # this tree and the parent, alternating
                sides.append((Path(args.parent) / "onitama-alphazero_amd", "parent_runs"))
            for pkg, key in ab.schedule(sides, 2 if T == 0 else 1):
                one("throughput", games, T, pkg, key)
        if args.parent and 0 in temps:  # T = 0 against the parent, in plies/s
            off = [r["median_plies_per_s"] for r in doc["runs"] if r["games"] == games and r["temperature_plies"] == 0]
            v = ab.spread_verdict(off, [r["median_plies_per_s"] for r in doc["parent_runs"] if r["games"] == games],
                                  higher_is_better=True)
            doc["off_against_parent"][str(games)] = {
                "this_tree_median_plies_per_s": v["mine"], "parent_median_plies_per_s": v["other"],
                "parent_spread": v["other_spread"], "this_tree_slower_by": v["behind_by"], "accepted": v["accepted"]}
            run.save()
    if args.diversity_games > 0:
        for T in temps:
            one("diversity", args.diversity_games, T, None, "diversity")
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
