#!/usr/bin/env python3
"""The device replay buffer (onitama_az.replay, csrc/oaz_replay.hip): what it costs to keep an iteration's samples on
the device and to merge equal positions, against the host round trip the loop does by default; how much of a
window is repetition; and what an epoch looks like on the merged buffer. Measurement tool; bench.py is the
flagship's and is not touched. What merging is worth in playing strength is not measured here.

The flagship's engine (3-block network, random-init weights seed 0, fp16x3 split, 400 simulations, root noise).
Every measurement runs in a child process of its own under `timeout`, one at a time; the first child without exit
status 0 and a result ends the whole run (tools/ab.py).

(a) Data handling (`--sizes`, default 4 096 and 65 536 games per iteration; fixed deck, T = 0). One engine plays
the iteration's games three times (selfplay_run with cap 0: the same games, the same records). After the first
the records go the way the loop sends them by default: samples_fetch to the host, then Trainer.load_samples
(after a load of as many records, so that no allocation is timed). After the second: append_engine + view(0);
after the third: append_engine + view(1) (after an append and a merged view of as many distinct records, so that
no allocation is timed). The host's monotonic clock around the calls, each of which returns synchronised. Then
`--reps` more view(1) of the same window: wall time and the kernels' time by phase (HIP events).

(b) Merged share (`--share-games`, default 4 096 per iteration, four iterations with the loop's seeds): T = 0 and
T = 8, fixed deck and dealt decks; after every iteration the records, the groups and the largest group of a
window of one and of a window of four iterations.

(c) Training outcome on one fixed buffer (the first iteration of (b) with T = 0 and the fixed deck): a 3-block
network from random-init weights, batch 512, `--epochs` epochs on view(0) and on view(1), the same seed: steps
per epoch and every epoch's loss.

`--parent DIR`: a checkout of the parent commit, built; a default-options loop (2 iterations of 1 024 games, 3
blocks, batch 512, 2 epochs) is then timed with DIR's package and library alternating with this tree's (this
tree, parent, this tree, parent), and this tree is accepted when its slower run is no slower than the parent's
slower run by more than the parent's two runs differ from each other.

usage: python tools/replay_bench.py [--out profiles/replay_<date>.json] [--sizes 4096,65536] [--reps 5]
                                    [--share-games 4096] [--epochs 8] [--parent DIR]"""
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
SEED = 20260101


def _pkg(args):
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))


def _engine_kw(_abi, games, temperature, fixed_deck, seed):
    kw = dict(games=games, sims=400, blocks=3, c_puct=5.0, train_noise=1, max_plies=150, evaluator=_abi.EVAL_NN,
              precision=_abi.FP32_SPLIT16, seed=seed, compact=0, parts=0, sample_capacity=games * 152,
              temperature_plies=temperature)
    if fixed_deck:
        kw.update(fixed_deck=1, deck=[0, 1, 2, 3, 4])
    return kw


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def child_handling(args) -> None:
    import numpy as np
    _pkg(args)
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.replay import ReplayBuffer
    from onitama_az.trainer import Trainer
    from onitama_az.weights import random_weights

    G = args.games
    with Engine(**_engine_kw(_abi, G, 0, True, SEED)) as e, Trainer(blocks=3, max_batch=512) as tr, \
            ReplayBuffer(capacity=G * 152) as buf:
        e.load_weights(random_weights(0, 3))
        t_play, _ = _ms(lambda: e.selfplay_run(G, cap=0))
        n = int(e.selfplay_stats().samples_ready)
        warm = np.zeros(n, dtype=_abi.SAMPLE_DTYPE)
        warm["state"]["kings"][:, 0] = np.arange(n)  # n distinct keys: every scratch array at its size
        tr.load_samples(warm)
        buf.append(warm)
        buf.view(merge=True)
        t_fetch, host = _ms(lambda: e.samples_fetch(n))
        t_load, _ = _ms(lambda: tr.load_samples(host))
        assert len(host) == n
        e.selfplay_run(G, cap=0)
        t_app0, n0 = _ms(lambda: buf.append_engine(e, 1))
        t_view0, v0 = _ms(lambda: buf.view(merge=False))
        e.selfplay_run(G, cap=0)
        t_app1, n1 = _ms(lambda: buf.append_engine(e, 2))
        t_view1, v1 = _ms(lambda: buf.view(merge=True))
        assert n0 == n1 == n and v0[1] == n
        phases, st = buf.merge_times(), buf.stats()
        again = []
        for _ in range(args.reps):
            ms, _ = _ms(lambda: buf.view(merge=True))
            again.append(dict(buf.merge_times(), wall_ms=ms))
        same = buf.fetch(merge=False)[0].tobytes() == host.tobytes()
    out = {"games": G, "records": n, "selfplay_ms": t_play, "records_equal_the_fetched_ones": bool(same),
           "host_round_trip": {"samples_fetch_ms": t_fetch, "load_samples_ms": t_load, "total_ms": t_fetch + t_load},
           "device_plain": {"append_engine_ms": t_app0, "view0_ms": t_view0, "total_ms": t_app0 + t_view0},
           "device_merged": {"append_engine_ms": t_app1, "view1_ms": t_view1, "total_ms": t_app1 + t_view1,
                             "kernel_ms_by_phase": phases, "kernel_ms": sum(phases.values())},
           "unique": int(st.unique), "unique_share": st.unique / max(1, n), "max_mult": int(st.max_mult),
           "probes": int(st.probes), "probes_per_record": st.probes / max(1, n),
           "view1_again": again, "view1_again_median_wall_ms": statistics.median(a["wall_ms"] for a in again),
           "view1_again_median_kernel_ms_by_phase": {k: statistics.median(a[k] for a in again) for k in _abi.REPLAY_PHASES}}
    print("RESULT " + json.dumps(out), flush=True)


def child_share(args) -> None:
    _pkg(args)
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.replay import ReplayBuffer
    from onitama_az.weights import random_weights

    G, rows = args.games, []
    with ReplayBuffer(capacity=4 * G * 152, window=1) as one, ReplayBuffer(capacity=4 * G * 152, window=4) as four:
        for it in range(1, 5):
            with Engine(**_engine_kw(_abi, G, args.temperature, args.fixed_deck, SEED + it)) as e:
                e.load_weights(random_weights(0, 3))
                e.selfplay_run(G, cap=0)
                one.append_engine(e, it)
            ptr, n, _ = one.view(merge=False)
            four.append_device(ptr, n, it)
            row = {"iteration": it}
            for name, buf in (("window_1", one), ("window_4", four)):
                buf.view(merge=True)
                st = buf.stats()
                row[name] = {"records": int(st.records), "unique": int(st.unique), "unique_share": st.unique / max(1, st.records),
                             "max_mult": int(st.max_mult), "segments": int(st.segments)}
            rows.append(row)
    print("RESULT " + json.dumps({"games_per_iteration": G, "temperature_plies": args.temperature,
                                  "fixed_deck": bool(args.fixed_deck), "iterations": rows}), flush=True)


def child_train(args) -> None:
    _pkg(args)
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.replay import ReplayBuffer
    from onitama_az.trainer import Trainer, train_epochs_device
    from onitama_az.weights import random_weights

    G, out = args.games, {}
    with ReplayBuffer(capacity=G * 152) as buf:
        with Engine(**_engine_kw(_abi, G, 0, True, SEED + 1)) as e:
            e.load_weights(random_weights(0, 3))
            e.selfplay_run(G, cap=0)
            buf.append_engine(e, 1)
        for merge in (False, True):
            ptr, n, _ = buf.view(merge=merge)
            with Trainer(blocks=3, max_batch=512) as tr:
                tr.set_weights(random_weights(0, 3))
                ms, hist = _ms(lambda: train_epochs_device(tr, ptr, n, epochs=args.epochs, batch=512, seed=7))
            out["merged" if merge else "plain"] = {
                "records": n, "steps_per_epoch": hist[0].steps if hist else 0, "epochs": len(hist), "train_ms": ms,
                "loss": [h.loss for h in hist], "value_loss": [h.value for h in hist], "policy_loss": [h.policy for h in hist]}
    print("RESULT " + json.dumps(dict(out, games=G, batch=512, blocks=3,
                                      note="the two losses are against different targets: the merged buffer's are "
                                           "means over the copies of a position")), flush=True)


def child_loop(args) -> None:
    import tempfile
    _pkg(args)
    from onitama_az.game import Deck  # noqa: F401  (the package as the loop's user imports it)
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train

    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=3),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=400, train=True), iterations=2,
                     training_epochs=2, train_batch_size=512, self_play_game_amnt=1024, save_checkpoint=99,
                     evaluation_checkpoint=99)
    with tempfile.TemporaryDirectory() as tmp:
        ms, st = _ms(lambda: train(cfg, folder=tmp))
    print("RESULT " + json.dumps({"side": "parent" if args.pkg else "this tree", "loop_ms": ms, "loss": st.loss,
                                  "positions": [g["positions_retrieved"] for g in st.games_played]}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--share-games", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", default=None, choices=["handling", "share", "train", "loop"], help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=4096, help=argparse.SUPPRESS)
    ap.add_argument("--temperature", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--fixed-deck", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"handling": child_handling, "share": child_share, "train": child_train, "loop": child_loop}[args.child](args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"replay_{date}.json")
    doc = {"tool": "tools/replay_bench.py", "date": date,
           "method": "per measurement a child process; the flagship's engine (3 blocks, 400 simulations, random-init "
                     "weights, root noise). handling: host clock around calls that return synchronised, no allocation "
                     "timed; kernel times by HIP events on the buffer's stream (the key phase includes the table's fill). "
                     "share: groups / records of the merged view. train: batch 512, 3 blocks from random-init weights",
           "out_of_scope": "what merging and a longer window are worth in playing strength",
           "handling": [], "merged_share": [], "training": None, "loop": [], "loop_parent": [], "loop_against_parent": None}
    run = ab.Run(out, doc)
    me = [sys.executable, str(Path(__file__).resolve()), "--reps", str(args.reps), "--epochs", str(args.epochs)]

    def one(what, extra, limit=600):
        res = run.child(what, me + extra, limit)[-1]
        print(f"{what}: done", flush=True)
        run.save()
        return res

    for g in (int(x) for x in args.sizes.split(",") if x):
        doc["handling"].append(one(f"handling {g}", ["--child", "handling", "--games", str(g)]))
    for temp in (0, 8):
        for fixed in (1, 0):
            doc["merged_share"].append(one(f"share T={temp} fixed_deck={fixed}", [
                "--child", "share", "--games", str(args.share_games), "--temperature", str(temp), "--fixed-deck", str(fixed)]))
    doc["training"] = one("train", ["--child", "train", "--games", str(args.share_games)])
    if args.parent:
        sides = [(None, "loop"), (str(Path(args.parent) / "onitama-alphazero_amd"), "loop_parent")]
        for pkg, key in ab.schedule(sides, 2):
            doc[key].append(one(f"loop {key}", ["--child", "loop"] + (["--pkg", pkg] if pkg else [])))
        v = ab.spread_verdict([r["loop_ms"] for r in doc["loop"]], [r["loop_ms"] for r in doc["loop_parent"]],
                              higher_is_better=False)
        doc["loop_against_parent"] = {"this_tree_loop_ms": v["mine"], "parent_loop_ms": v["other"],
                                      "parent_spread_ms": v["other_spread"], "this_tree_slower_by_ms": v["behind_by"],
                                      "accepted": v["accepted"]}
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
