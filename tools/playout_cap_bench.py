#!/usr/bin/env python3
"""Self-play with playout cap randomization (Engine(playout_cap=(n, P))) beside self-play without, on one GPU: what a
ply costs when most plies stop after n playouts, and where the time goes. Measurement tool; bench.py is the
flagship's and is not touched.

The flagship's engine (3-block network, random-init weights seed 0, fp16x3 split, 400 simulations, root noise, fixed
deck, compact 0, automatic parts). Every configuration runs in a child process of its own under `timeout`, one at a
time; the first child without exit status 0 and a result ends the whole run (tools/ab.py).

Throughput (`--sizes`, default 65 536 and 4 096 games; caps in `--caps`, "off" or n:P; `--big-caps` are run at the
first size only): staggered starts, `--warmup` plies, then `--reps` timed windows of `--plies` plies each, the host's
monotonic clock around selfplay_step + sync, as tools/temperature_bench.py. Reported per configuration: plies/s per
window with median, minimum and maximum; the full and fast plies of the windows (oaz_selfplay_playout_cap_stats) and
the measured full share; records/s = full plies/s (every full ply becomes a record when its game ends; without a cap
every ply is one). Then one more window with the engine's event timing on every launch: the network kernel's busy
time per ply (the union of its launches' intervals over the game parts' streams) and its share of that same window's
ply. The events slow the window by several percent, more where the steps are short, so it is not among the
throughput windows and the share, not the milliseconds, is the figure to read; where the whole search is one launch
per noise chunk (k_search_grp: cap off at 4 096 games) the network is not a launch of its own and both are null.

Game length (`--length-games`, default 4 096; each cap of `--caps`): the games 0 .. n-1 played to their end
(selfplay_run, every slot one game): mean plies and mean records per game. games/s of a throughput run is then
derived, not measured: plies/s divided by the mean plies per game under the same cap.

`--parent DIR`: a checkout of the parent commit, built; "off" is then also measured with DIR's package and library,
alternating with this tree's (this tree, parent, this tree, parent), and both are recorded. Off is accepted when
this tree's slower run is no slower than the parent's slower run by more than the parent's two runs differ.

usage: python tools/playout_cap_bench.py [--out profiles/playout_cap_<date>.json] [--sizes 65536,4096]
                                         [--caps off,100:16384] [--big-caps 50:16384,100:32768] [--sims 400]
                                         [--warmup 14] [--plies 4] [--reps 5] [--parent DIR] [--length-games 4096]"""
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


def parse_cap(text):
    """"off" -> None, "n:P" -> (n, P)."""
    if text == "off":
        return None
    n, _, p = text.partition(":")
    return int(n), int(p or 16384)


def engine_kw(_abi, args, **more):
    kw = dict(games=args.games, sims=args.sims, blocks=3, c_puct=5.0, train_noise=1, max_plies=150,
              evaluator=_abi.EVAL_NN, precision=_abi.FP32_SPLIT16, fixed_deck=1, deck=[0, 1, 2, 3, 4], seed=20260101,
              compact=0, parts=0, **more)
    if parse_cap(args.cap):  # (the parent's engine has no such setting)
        kw["playout_cap"] = parse_cap(args.cap)
    return kw


def child_throughput(args) -> None:
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    cap = parse_cap(args.cap)
    with Engine(**engine_kw(_abi, args, sample_capacity=args.games * 8, stagger=min(12, args.warmup))) as e:
        e.load_weights(random_weights(0, 3))
        e.selfplay_reset()
        for _ in range(args.warmup):
            e.selfplay_step(1)
        e.sync()
        st0 = e.selfplay_stats()
        cs0 = e.playout_cap_stats() if cap else (0, 0)
        rates, secs = [], 0.0
        for _ in range(args.reps):
            e.samples_fetch(args.games * 8)  # (the buffer never fills)
            e.sync()
            t0 = time.perf_counter()
            e.selfplay_step(args.plies)
            e.sync()
            dt = time.perf_counter() - t0
            secs += dt
            rates.append(args.games * args.plies / dt)
        st1 = e.selfplay_stats()
        cs1 = e.playout_cap_stats() if cap else (0, 0)
        moves = int(st1.moves - st0.moves)
        full, fast = (cs1[0] - cs0[0], cs1[1] - cs0[1]) if cap else (moves, 0)
        # one more window with every launch timed
        e.samples_fetch(args.games * 8)
        e.kernel_times_reset()
        e.set_timing(True)
        e.sync()
        t0 = time.perf_counter()
        e.selfplay_step(args.plies)
        e.sync()
        timed_ply_ms = 1e3 * (time.perf_counter() - t0) / args.plies
        e.set_timing(False)
        kt = e.kernel_times()
        nn_ms_per_ply = kt.nn_busy_ms / args.plies if kt.nn_n else None
        out = {"games": args.games, "sims": args.sims, "cap": args.cap, "plies_per_window": args.plies,
               "plies_per_s": [round(r, 1) for r in rates], "median_plies_per_s": statistics.median(rates),
               "min_plies_per_s": min(rates), "max_plies_per_s": max(rates), "ms_per_ply": 1e3 * secs / (args.reps * args.plies),
               "moves": moves, "full_plies": int(full), "fast_plies": int(fast), "full_share": full / max(1, full + fast),
               "records_per_s": full / secs, "playouts": int(st1.search.sims - st0.search.sims),
               "nn_evals": int(st1.search.nn_evals - st0.search.nn_evals),
               "timed_window": {"ms_per_ply": timed_ply_ms, "nn_busy_ms_per_ply": nn_ms_per_ply,
                                "nn_share_of_ply": nn_ms_per_ply / timed_ply_ms if kt.nn_n else None,
                                "parts": int(kt.parts), "nn_launches_timed": int(kt.nn_n)}}
    print("RESULT " + json.dumps(out), flush=True)


def child_length(args) -> None:
    sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    n = args.games
    with Engine(**engine_kw(_abi, args, sample_capacity=n * 152)) as e:
        e.load_weights(random_weights(0, 3))
        t0 = time.perf_counter()
        _, st = e.selfplay_run(n, cap=0)
        secs = time.perf_counter() - t0
        cs = e.playout_cap_stats()
        records = int(st.samples_ready)
    out = {"games": n, "sims": args.sims, "cap": args.cap, "games_finished": int(st.games_finished),
           "plies": int(st.moves), "records": records, "mean_plies_per_game": st.moves / max(1, int(st.games_finished)),
           "mean_records_per_game": records / max(1, int(st.games_finished)), "full_plies": cs[0], "fast_plies": cs[1],
           "games_cut": int(st.games_cut), "red_wins": int(st.red_wins), "blue_wins": int(st.blue_wins),
           "samples_dropped": int(st.samples_dropped), "seconds": round(secs, 2)}
    print("RESULT " + json.dumps(out), flush=True)


def child_cmd(args, mode, games, cap, pkg=None) -> list:
    """The command of one configuration's child process."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", mode, "--games", str(games), "--cap", cap,
           "--sims", str(args.sims), "--warmup", str(args.warmup), "--plies", str(args.plies), "--reps", str(args.reps)]
    return cmd + (["--pkg", str(pkg)] if pkg else [])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="65536,4096")
    ap.add_argument("--caps", default="off,100:16384")
    ap.add_argument("--big-caps", default="50:16384,100:32768", help="more caps, at the first size only")
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=14)
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--length-games", type=int, default=4096, help="0: no game-length runs")
    ap.add_argument("--child", default=None, choices=["throughput", "length"], help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cap", default="off", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_throughput(args) if args.child == "throughput" else child_length(args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"playout_cap_{date}.json")
    sizes = [int(x) for x in args.sizes.split(",")]
    caps = [c for c in args.caps.split(",") if c]
    big = [c for c in args.big_caps.split(",") if c]
    doc = {"tool": "tools/playout_cap_bench.py", "date": date, "sims": args.sims, "warmup_plies": args.warmup,
           "method": "per configuration a child process. throughput: staggered starts, warm-up plies, then `reps` windows "
                     "of `plies_per_window` plies, host clock around selfplay_step + sync; plies/s = games x plies / "
                     "window; records/s = full plies / the windows' seconds; then one window with event timing on every "
                     "launch: nn_busy_ms_per_ply = the union of the network launches' intervals / plies, its share of "
                     "that window's ply (null where the search is one launch per noise chunk). "
                     "length: selfplay_run of games 0 .. n-1 on n slots. games_per_s = median plies/s / the mean plies "
                     "per game under the same cap (derived)",
           "tile_count_prediction": "65 536 games, 400/100 playouts, a quarter of the plies full: 100 x 16 + 300 x 4 = "
                                    "2 800 rounds of 16-position tiles per ply instead of 6 400 (a count, not a measurement)",
           "lengths": [], "runs": [], "parent_runs": [], "off_against_parent": {}, "summary": []}
    run = ab.Run(out, doc)

    def one(mode, games, cap, pkg, key):
        what = f"{mode} games {games} cap {cap} {'parent' if pkg else 'this tree'}"
        res = run.child(what, child_cmd(args, mode, games, cap, pkg=pkg), 900)[-1]
        print(f"{what}: {round(res['median_plies_per_s'], 1) if mode == 'throughput' else res['mean_plies_per_game']}",
              flush=True)
        doc[key].append(res)
        run.save()
        return res

    if args.length_games > 0:
        for cap in caps + big:
            one("length", args.length_games, cap, None, "lengths")
    plies_per_game = {r["cap"]: r["mean_plies_per_game"] for r in doc["lengths"]}
    for k, games in enumerate(sizes):
        for cap in caps + (big if k == 0 else []):
            sides = [(None, "runs")]
            if cap == "off" and args.parent:  # this tree and the parent, alternating
                sides.append((Path(args.parent) / "onitama-alphazero_amd", "parent_runs"))
            for pkg, key in ab.schedule(sides, 2 if cap == "off" else 1):
                r = one("throughput", games, cap, pkg, key)
                if pkg is None:
                    t = r["timed_window"]
                    doc["summary"].append({
                        "games": games, "cap": cap, "plies_per_s": r["median_plies_per_s"],
                        "games_per_s": r["median_plies_per_s"] / plies_per_game[cap] if cap in plies_per_game else None,
                        "records_per_s": r["records_per_s"], "full_share": r["full_share"],
                        "nn_busy_ms_per_ply": t["nn_busy_ms_per_ply"], "nn_share_of_ply": t["nn_share_of_ply"]})
                    run.save()
        if args.parent and "off" in caps:  # cap off against the parent, in plies/s
            off = [r["median_plies_per_s"] for r in doc["runs"] if r["games"] == games and r["cap"] == "off"]
            v = ab.spread_verdict(off, [r["median_plies_per_s"] for r in doc["parent_runs"] if r["games"] == games],
                                  higher_is_better=True)
            doc["off_against_parent"][str(games)] = {
                "this_tree_median_plies_per_s": v["mine"], "parent_median_plies_per_s": v["other"],
                "parent_spread": v["other_spread"], "this_tree_slower_by": v["behind_by"], "accepted": v["accepted"]}
            run.save()
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
