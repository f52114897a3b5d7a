#!/usr/bin/env python3
"""Throughput and latency of the batched alpha-beta search (oaz_alphabeta_search) on one GPU, beside the
CPU restatement (tests/c/alphabeta_ref.c) on the same roots. Measurement tool; bench.py is the flagship's.

  - max_depth 4 (the arena's opponent, 3 plies): G = 4 096 and 65 536 roots, start-of-game (seeded deals)
    and mid-game (10-30 random plies of seeded deals, non-terminal with a legal move);
  - max_depth 6 (the default, 5 plies): one mid-game root per call, for latency;
  - the restatement on one thread and on 16 threads over a sample of the same roots.

Method: every shape is warmed up, then timed `--reps` times with the host's monotonic clock around the whole
call (upload, launch, stream synchronise, download; the call returns after its stream is idle), and the
median is reported with the minimum and maximum. Writes one JSON file.

usage: python tools/alphabeta_bench.py [--out profiles/alphabeta_<date>.json] [--reps 7] [--pit GAMES] [--deep]
  --deep measures the split search instead (oaz_alphabeta_generate_move, untimed; profiles/alphabeta_deep_<date>.json),
  by the same method: one mid-game root per call (the latency roots above) at max_depth 6 and 8 for split 1, 2, 3
  and auto, oaz_alphabeta_search at max_depth 6 and the one-thread restatement on the same roots, 4 096 roots at
  max_depth 4 on both paths, with the items, positions and elapsed_ms of each; and the positions per second one
  lane sustains, from the split-1 max_depth-8 calls (the call lasts as long as its longest item, whose positions
  the restatement counts from that root child).
  --pit GAMES also times Evaluator.pit(alphabeta=True) against pit(alphabeta=False) at game_amnt = GAMES
  (as tools/pit_timing.py: trained 3-block network vs a random one, concurrent fights)."""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from onitama_az import _abi  # noqa: E402
from onitama_az.alpha_beta import alpha_beta_search  # noqa: E402
from onitama_az.game import Deck, initial_state_np, movegen_batch, step_batch  # noqa: E402


def start_roots(n: int, seed: int) -> np.ndarray:
    return np.concatenate([initial_state_np(Deck.default(seed, k).indices()) for k in range(n)])


def midgame_roots(n: int, seed: int, lo: int = 10, hi: int = 30) -> np.ndarray:
    """n positions after lo..hi random plies of seeded deals (GPU rules), each non-terminal with a legal move:
    a game that ends or gets stuck earlier is replayed from a fresh deal."""
    rng = np.random.default_rng(seed)
    out, deal = [], 0
    while sum(len(o) for o in out) < n:
        m = max(n - sum(len(o) for o in out), 256)
        s = np.concatenate([initial_state_np(Deck.default(seed, deal + k).indices()) for k in range(m)])
        deal += m
        target = rng.integers(lo, hi + 1, m)
        ok = np.ones(m, dtype=bool)
        for ply in range(hi):
            idx = np.nonzero(ok & (target > ply))[0]
            if len(idx) == 0:
                break
            sub = np.ascontiguousarray(s[idx])
            moves, counts = movegen_batch(sub)
            ok[idx[counts == 0]] = False
            keep = counts > 0
            idx, sub, moves, counts = idx[keep], np.ascontiguousarray(sub[keep]), moves[keep], counts[keep]
            res = step_batch(sub, moves[np.arange(len(idx)), (rng.random(len(idx)) * counts).astype(np.int64)])
            s[idx] = sub
            ok[idx[(res == _abi.RED_WIN) | (res == _abi.BLUE_WIN)]] = False
        fin = np.nonzero(ok)[0]
        _, counts = movegen_batch(np.ascontiguousarray(s[fin]))
        out.append(s[fin[counts > 0]])
    return np.ascontiguousarray(np.concatenate(out)[:n])


def timed(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": reps}


def cpu_rate(ref, roots: np.ndarray, max_depth: int, threads: int):
    """The restatement over `roots` split evenly over `threads` host threads (ctypes releases the GIL)."""
    n = len(roots)
    mv = np.zeros(n, dtype=_abi.MOVE_DTYPE)
    sc = np.zeros(n, dtype=np.int32)
    pos = np.zeros(n, dtype=np.int64)
    cuts = np.linspace(0, n, threads + 1).astype(int)

    def shard(k):
        a, b = int(cuts[k]), int(cuts[k + 1])
        rc = ref.abref_search_batch(_abi.ptr(roots[a:b]), b - a, max_depth, _abi.ptr(mv[a:b]), _abi.ptr(sc[a:b]),
                                    _abi.ptr(pos[a:b]))
        assert rc == 0

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(shard, range(threads)))
    dt = time.perf_counter() - t0
    return {"threads": threads, "roots": n, "seconds": dt, "roots_per_s": n / dt, "positions": int(pos.sum()),
            "positions_per_s": float(pos.sum()) / dt}, mv, sc


def cpu_one(ref, root: np.ndarray, max_depth: int):
    """(seconds, positions) of the restatement's search of one root on this thread."""
    mv = np.zeros(1, dtype=_abi.MOVE_DTYPE)
    sc = np.zeros(1, dtype=np.int32)
    pos = np.zeros(1, dtype=np.int64)
    t0 = time.perf_counter()
    rc = ref.abref_search_batch(_abi.ptr(root), 1, max_depth, _abi.ptr(mv), _abi.ptr(sc), _abi.ptr(pos))
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, int(pos[0]), mv, sc


def longest_item(ref, root: np.ndarray, max_depth: int) -> int:
    """Positions of the longest item of a split-1 search of `root`: a lane walks a root child's subtree as the
    sequential search does from that child, so the restatement from the child to max_depth - 1 counts the same
    positions (a child reached by a winning move is one position)."""
    moves, counts = movegen_batch(root)
    n = int(counts[0])
    kids = np.ascontiguousarray(np.repeat(root, n))
    res = step_batch(kids, np.ascontiguousarray(moves[0, :n]))  # (to_move switches)
    return max(1 if res[k] in (_abi.RED_WIN, _abi.BLUE_WIN) else cpu_one(ref, kids[k:k + 1], max_depth - 1)[1]
               for k in range(n))


def deep(args, ref) -> int:
    """The split search (oaz_alphabeta_generate_move) beside oaz_alphabeta_search and the restatement: one mid-game
    root per call at max_depth 6 and 8 for split 1, 2, 3 and auto, and 4 096 roots at max_depth 4 on both paths."""
    from onitama_az.alpha_beta import alpha_beta_generate_move
    pool = midgame_roots(65536, 7201)  # the roots of latency_max_depth6_one_midgame_root (alphabeta_<date>.json)
    n_lat = args.deep_roots
    out = {"tool": "tools/alphabeta_bench.py --deep", "date": f"{datetime.date.today():%Y-%m-%d}",
           "clock": "time.perf_counter around the whole call (upload, every launch and read-back of the levels, "
                    "download, per-call hipMalloc/hipFree and stream create/destroy); elapsed_ms is the call's own",
           "reps": args.reps, "warmup": 2, "one_midgame_root": [], "batch_4096_max_depth4": []}
    alpha_beta_generate_move(pool[:1], max_depth=4)
    for depth in (6, 8):
        cpu = [cpu_one(ref, np.ascontiguousarray(pool[i:i + 1]), depth) for i in range(n_lat)] if ref is not None else None
        paths = [("generate_move", s) for s in (1, 2, 3, 0)] + ([("search", None)] if depth == 6 else [])
        for path, split in paths:
            rows = []
            for i in range(n_lat):
                one = np.ascontiguousarray(pool[i:i + 1])
                if path == "search":
                    r, t = timed(lambda: alpha_beta_search(one, max_depth=depth), 2, args.reps)
                    row = {**t, "positions": int(r.stats.positions)}
                else:
                    r, t = timed(lambda: alpha_beta_generate_move(one, max_depth=depth, split=split), 2, args.reps)
                    row = {**t, "positions": int(r.stats.positions), "items": int(r.stats.items),
                           "split_used": int(r.stats.split), "elapsed_ms": float(r.stats.elapsed_ms)}
                    if cpu is not None:
                        row["equal_to_cpu"] = bool(r.moves.tobytes() == cpu[i][2].tobytes() and r.scores[0] == cpu[i][3][0])
                    if split == 1 and depth == 8 and ref is not None:  # few lanes, each long: the per-lane rate
                        row["longest_item_positions"] = longest_item(ref, one, depth)
                        row["lane_positions_per_s"] = row["longest_item_positions"] / t["median_s"]
                if cpu is not None:
                    row.update(cpu1_s=cpu[i][0], cpu1_positions=cpu[i][1], x_cpu1=cpu[i][0] / t["median_s"])
                rows.append(row)
            sec = {"max_depth": depth, "path": path, "split": split, "roots": rows,
                   "median_of_medians_s": statistics.median(x["median_s"] for x in rows),
                   "min_of_medians_s": min(x["median_s"] for x in rows),
                   "max_of_medians_s": max(x["median_s"] for x in rows)}
            if cpu is not None:
                sec["cpu1_median_s"] = statistics.median(c[0] for c in cpu)
                sec["x_cpu1_median"] = sec["cpu1_median_s"] / sec["median_of_medians_s"]
            if "lane_positions_per_s" in rows[0]:
                sec["lane_positions_per_s_median"] = statistics.median(x["lane_positions_per_s"] for x in rows)
            out["one_midgame_root"].append(sec)
            print(json.dumps({k: v for k, v in sec.items() if k != "roots"}), flush=True)
    roots = np.ascontiguousarray(pool[:4096])
    for path, fn in (("search", lambda: alpha_beta_search(roots, max_depth=4)),
                     ("generate_move", lambda: alpha_beta_generate_move(roots, max_depth=4))):
        r, t = timed(fn, 2, args.reps)
        row = {"path": path, "G": 4096, "max_depth": 4, **t, "roots_per_s": 4096 / t["median_s"],
               "positions": int(r.stats.positions)}
        if path == "generate_move":
            row.update(items=int(r.stats.items), split_used=int(r.stats.split), elapsed_ms=float(r.stats.elapsed_ms))
        out["batch_4096_max_depth4"].append(row)
        print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-roots", type=int, default=4096)
    ap.add_argument("--pit", type=int, default=0)
    ap.add_argument("--pit-sims", type=int, default=400)
    ap.add_argument("--deep", action="store_true", help="measure the split search (profiles/alphabeta_deep_<date>.json)")
    ap.add_argument("--deep-roots", type=int, default=8)
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / f"alphabeta_{'deep_' if args.deep else ''}{datetime.date.today():%Y%m%d}.json")
    if _abi.device_count() == 0:
        raise SystemExit("no GPU: this tool measures on one")
    import make_alphabeta_kats as gen
    if args.deep:
        with tempfile.TemporaryDirectory() as tmp:
            ref = gen.build_ref(Path(tmp))
            if ref is not None:
                ref.abref_search_batch.restype = C.c_int
                ref.abref_search_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            return deep(args, ref)
    with tempfile.TemporaryDirectory() as tmp:
        ref = gen.build_ref(Path(tmp))
        if ref is not None:
            ref.abref_search_batch.restype = C.c_int
            ref.abref_search_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        out = {"tool": "tools/alphabeta_bench.py", "date": f"{datetime.date.today():%Y-%m-%d}",
               "clock": "time.perf_counter around oaz_alphabeta_search (upload + kernel + stream synchronise + "
                        "download + per-call hipMalloc/hipFree and stream create/destroy)",
               "reps": args.reps, "throughput_max_depth4": [], "cpu_restatement": []}
        for kind, make in (("start", start_roots), ("midgame", midgame_roots)):
            pool = make(65536, 7201)
            for G in (4096, 65536):
                roots = np.ascontiguousarray(pool[:G])
                r, t = timed(lambda: alpha_beta_search(roots, max_depth=4), 2, args.reps)
                row = {"roots_kind": kind, "G": G, **t, "roots_per_s": G / t["median_s"],
                       "positions": int(r.stats.positions), "positions_per_s": r.stats.positions / t["median_s"],
                       "max_positions_per_root": int(r.stats.max_positions_per_root)}
                out["throughput_max_depth4"].append(row)
                print(json.dumps(row), flush=True)
            if ref is not None:
                sample = np.ascontiguousarray(pool[:args.cpu_roots])
                gpu = alpha_beta_search(sample, max_depth=4)
                for threads in (1, 16):
                    c, mv, sc = cpu_rate(ref, sample, 4, threads)
                    c.update(roots_kind=kind, max_depth=4,
                             equal_to_gpu=bool(mv.tobytes() == gpu.moves.tobytes() and np.array_equal(sc, gpu.scores)))
                    out["cpu_restatement"].append(c)
                    print(json.dumps(c), flush=True)
            if kind == "midgame":
                lat = []
                for i in range(8):
                    one = np.ascontiguousarray(pool[i:i + 1])
                    r, t = timed(lambda: alpha_beta_search(one, max_depth=6), 2, args.reps)
                    lat.append({**t, "positions": int(r.stats.positions)})
                out["latency_max_depth6_one_midgame_root"] = {
                    "roots": lat, "median_of_medians_s": statistics.median(x["median_s"] for x in lat),
                    "max_of_medians_s": max(x["median_s"] for x in lat)}
                print(json.dumps(out["latency_max_depth6_one_midgame_root"]), flush=True)
                if ref is not None:
                    c, _, _ = cpu_rate(ref, np.ascontiguousarray(pool[:8]), 6, 1)
                    c.update(roots_kind=kind, max_depth=6)
                    out["cpu_restatement"].append(c)
        for row in out["throughput_max_depth4"]:  # GPU over the restatement on 16 threads, per kind of roots
            cpu = [c for c in out["cpu_restatement"] if c["roots_kind"] == row["roots_kind"] and c["max_depth"] == 4
                   and c["threads"] == 16]
            if cpu:
                row["x_cpu16_roots_per_s"] = row["roots_per_s"] / cpu[0]["roots_per_s"]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    if args.pit:  # (the search figures are on disk before the long part starts)
        out["pit"] = pit_ratio(args.pit, args.pit_sims)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)
    return 0


def pit_ratio(games: int, sims: int) -> dict:
    from onitama_az.evaluator import Evaluator, EvaluatorConfig
    from onitama_az.mcts import ConvResNet, ConvResNetConfig
    trained = np.load(ROOT / "tests" / "golden" / "weights_3block_trained.npy")
    new = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), weights=trained)
    best = ConvResNet(ConvResNetConfig(resnet_block_amnt=3), seed=7)
    ev = Evaluator(EvaluatorConfig(game_amnt=games, max_plies=150, seed=3), best, new)
    ev.pit(sims=8, concurrent=True, alphabeta=True)  # warm-up: engines, kernels, thread pool
    res = {"game_amnt": games, "sims": sims, "without_s": [], "with_s": []}
    for ab in (False, True, False, True):  # alternating, same process
        t0 = time.perf_counter()
        pit, _ = ev.pit(sims=sims, concurrent=True, alphabeta=ab)
        res["with_s" if ab else "without_s"].append(round(time.perf_counter() - t0, 3))
        if ab:
            f = pit.alphabeta_fight
            res["alphabeta_fight"] = {"winrate_new": f.winrate, "plies_max": max(f.plies),
                                      "wins": f.general.wins, "loses": f.general.loses, "draws": f.general.draws}
        print(json.dumps(res), flush=True)
    res["ratio_with_over_without"] = round(min(res["with_s"]) / min(res["without_s"]), 3)
    return res


if __name__ == "__main__":
    sys.exit(main())
