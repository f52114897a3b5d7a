#!/usr/bin/env python3
"""Agent-API latency of the leaf-parallel search (oaz_config.leaf_batch = L) beside the sequential search, on one
GPU. Measurement tool; bench.py is the flagship's and is not touched.

The flagship's engine (3-block network, fp16x3 split, c = sqrt 2, no root noise, no search_time budget) with the
trained 3-block weights (tests/golden/weights_3block_trained.npy). Two batch sizes: one root (the start position
and `--positions` seeded mid-game positions, each searched alone: "ms per move" is one oaz_search of one root) and
64 roots (64 seeded positions in one oaz_search: ms per move = that call), at 400 and 5 000 playouts, for
L in 0 (k_search_lat), 1, 2, 4, 8, 16 (k_search_par). Every (batch, playouts) pair runs in a child process of its
own under `timeout`, one at a time; the first child without exit status 0 and a result ends the whole run
(tools/ab.py).

Per configuration: one untimed search of every root set (code objects, first touches), then `--reps` timed
searches of each, the host's monotonic clock around oaz_search (upload + one launch + finalize + the copies back,
ending in a stream synchronise). Reported: ms per move as the median, minimum and maximum over all timed searches,
and the rounds (network passes), playouts and discarded walks per search (oaz_search_leaf_batch_stats).

`--parent DIR`: a checkout of the parent commit, built; L = 0 is then also measured with DIR's package and
library, alternating with this tree's (this tree, parent, this tree, parent): with leaf_batch off the engine must
run as the parent does. This tree's two runs measure every L, so each L has its own run-to-run spread.

`--fight N` (default 256, the MI355X's CU count; 0: none): one fight of N games, agent L = 8 against agent L = 0
on the same network at 400 playouts each, sides alternating, a deck dealt per game. Reported: wins, losses and
draws of the L = 8 agent and its win rate among decided games with the 95 % Wilson interval: what virtual loss
costs in strength at equal playouts. (The 3-block golden network is a small, briefly trained one: the figure
describes this network, not a strong one.)

usage: python tools/leaf_batch_bench.py [--out profiles/leaf_batch_<date>.json] [--reps 5] [--positions 5]
                                        [--batches 1,64] [--playouts 400,5000] [--ls 0,1,2,4,8,16] [--parent DIR]
                                        [--fight 256]"""
from __future__ import annotations

import argparse
import datetime
import json
import math
import statistics
import sys
import time
from pathlib import Path

import ab

ROOT = Path(__file__).resolve().parents[1]
WEIGHTS = ROOT / "tests" / "golden" / "weights_3block_trained.npy"
C_PUCT = math.sqrt(2.0)


def seeded_positions(n, seed):
    """n mid-game positions from seeded random play on the GPU rules (fixed deck, 4 .. 24 plies, none finished)."""
    import numpy as np
    from onitama_az import _abi
    from onitama_az.game import initial_state_np, movegen_batch, step_batch
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        s = initial_state_np([0, 1, 2, 3, 4])
        ok = True
        for _ in range(int(rng.integers(4, 25))):
            moves, counts = movegen_batch(s)
            if counts[0] == 0:
                ok = False
                break
            res = step_batch(s, moves[:1, int(rng.integers(0, counts[0]))])
            if res[0] in (_abi.RED_WIN, _abi.BLUE_WIN):
                ok = False
                break
        if ok and movegen_batch(s)[1][0] > 0:
            out.append(s.copy())
    return np.concatenate(out)


def child(args) -> None:
    """One (batch, playouts) pair, in this process: prints one JSON line per L."""
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))
    import numpy as np
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.game import initial_state_np

    w = np.load(WEIGHTS, allow_pickle=False)
    if args.batch == 1:
        pos = np.concatenate([initial_state_np([0, 1, 2, 3, 4]), seeded_positions(args.positions, 20261020)])
        sets = [np.ascontiguousarray(pos[i:i + 1]) for i in range(len(pos))]
    else:
        sets = [seeded_positions(args.batch, 20261021)]
    for L in [int(x) for x in args.ls.split(",")]:
        kw = dict(games=args.batch, sims=args.sims, blocks=3, c_puct=C_PUCT, train_noise=0, evaluator=_abi.EVAL_NN,
                  precision=_abi.FP32_SPLIT16)
        if L:  # (the parent's config has no such field)
            kw["leaf_batch"] = L
        with Engine(**kw) as e:
            e.load_weights(w)
            for roots in sets:
                e.search(roots)
            ms, rounds, playouts, disc = [], [], [], []
            for roots in sets:
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = e.search(roots)
                    ms.append(1e3 * (time.perf_counter() - t0))
                    assert r.stats.sims == args.sims * len(roots)
                    if L:
                        st = e.leaf_batch_stats()
                        rounds.append(st[0] / len(roots))
                        playouts.append(st[1] / len(roots))
                        disc.append(st[2] / len(roots))
            out = {"roots": args.batch, "playouts": args.sims, "leaf_batch": L, "searches_timed": len(ms),
                   "ms_per_move_median": statistics.median(ms), "ms_per_move_min": min(ms), "ms_per_move_max": max(ms),
                   "nn_fallbacks": e.nn_fallbacks()}
            if L:
                out.update(rounds_per_search=statistics.mean(rounds), playouts_per_search=statistics.mean(playouts),
                           discarded_walks_per_search=statistics.mean(disc))
            print("RESULT " + json.dumps(out), flush=True)


def fight_child(args) -> None:
    sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
    import numpy as np
    from onitama_az.evaluator import AlphaZeroAgent, EvaluatorConfig, fight
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNet, ConvResNetConfig

    model = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), weights=np.load(WEIGHTS, allow_pickle=False))
    cfg = dict(exploration_c=C_PUCT, max_playouts=args.sims, train=False, enforce_search_time=False)
    a = AlphaZeroAgent(AlphaZeroMctsConfig(leaf_batch=8, **cfg), model)
    b = AlphaZeroAgent(AlphaZeroMctsConfig(leaf_batch=0, **cfg), model)
    t0 = time.perf_counter()
    st = fight(EvaluatorConfig(game_amnt=args.fight, max_plies=150, seed=20261020), a, b)
    secs = time.perf_counter() - t0
    wins, loses, draws = st.general.wins, st.general.loses, st.general.draws
    n = wins + loses
    lo = hi = p = float("nan")
    if n:  # Wilson score interval, z = 1.96
        z, p = 1.96, wins / n
        mid, half = (p + z * z / (2 * n)) / (1 + z * z / n), z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / (1 + z * z / n)
        lo, hi = mid - half, mid + half
    print("RESULT " + json.dumps({
        "games": args.fight, "playouts": args.sims, "agent": "leaf_batch 8", "opponent": "leaf_batch 0",
        "wins": wins, "losses": loses, "draws": draws, "winrate_of_decided": p, "wilson95": [lo, hi],
        "as_red": [st.color[0].wins, st.color[0].loses, st.color[0].draws],
        "as_blue": [st.color[1].wins, st.color[1].loses, st.color[1].draws],
        "plies_total": int(sum(st.plies)), "seconds": secs,
        "caveat": "the small, briefly trained 3-block golden network; sides alternate, a deck dealt per game"}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=5)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--playouts", default="400,5000")
    ap.add_argument("--ls", default="0,1,2,4,8,16")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--fight", type=int, default=256)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fight-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--sims", type=int, default=400, help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.fight_child:
        return fight_child(args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"leaf_batch_{date}.json")
    doc = {"tool": "tools/leaf_batch_bench.py", "date": date, "reps": args.reps,
           "method": "per (roots, playouts) a child process; one untimed search of every root set, then `reps` timed "
                     "searches of each, host clock around oaz_search (ends in a stream synchronise); 1 root: the start "
                     "position and seeded mid-game positions, each searched alone; 64 roots: one call",
           "network": "3 blocks, tests/golden/weights_3block_trained.npy, fp16x3 split, c = sqrt 2",
           "runs": [], "parent_runs": [], "fight": None}

    run, me = ab.Run(out, doc), [sys.executable, str(Path(__file__).resolve())]
    for batch in [int(x) for x in args.batches.split(",")]:
        for sims in [int(x) for x in args.playouts.split(",")]:
            sides = [(None, "runs", args.ls)]
            if args.parent:  # this tree and the parent, alternating, twice each
                sides.append((Path(args.parent) / "onitama-alphazero_amd", "parent_runs", "0"))
            for k, (pkg, key, ls) in enumerate(ab.schedule(sides, 2 if args.parent else 1)):
                extra = ["--child", "--batch", str(batch), "--sims", str(sims), "--ls", ls, "--reps", str(args.reps),
                         "--positions", str(args.positions)] + (["--pkg", str(pkg)] if pkg else [])
                res = run.child(f"{'parent' if pkg else 'this tree'} roots {batch} playouts {sims}", me + extra, 600)
                for r in res:
                    r["run"] = k // 2
                    doc[key].append(r)
                    print(f"{'parent   ' if pkg else 'this tree'} roots {batch:3d} playouts {sims:5d} L {r['leaf_batch']:2d}: "
                          f"{r['ms_per_move_median']:8.3f} ms ({r['ms_per_move_min']:.3f} .. {r['ms_per_move_max']:.3f})"
                          + (f"  rounds {r['rounds_per_search']:.1f} discarded {r['discarded_walks_per_search']:.2f}"
                             if r["leaf_batch"] else ""), flush=True)
                run.save()
    if args.fight > 0:
        doc["fight"] = run.child("fight", me + ["--fight-child", "--fight", str(args.fight), "--sims", "400"], 900)[0]
        print(f"fight: {doc['fight']}", flush=True)
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
