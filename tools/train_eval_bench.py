#!/usr/bin/env python3
"""Held-out evaluation (Trainer.evaluate, onitama_az.holdout): what the eval-mode pass and the
split's kernel cost next to a training step, and what the loop's held-out metrics look like over a few iterations
with and without the reflection and merging options. Measurement tool; bench.py is the flagship's and is not
touched. No playing strength is measured here: the metrics say how well a network predicts self-play targets of
positions it was not trained on, not how it plays.

Every measurement runs in a child process of its own under `timeout`, one at a time; the first child without exit
status 0 and a result ends the whole run (tools/ab.py).

(a) Throughput (`--sizes`, default 4 096 and 65 536 games). One iteration of the flagship's self-play (3-block
random-init network seed 0, fp16x3, 400 simulations, root noise, fixed deck) goes device to device into a
ReplayBuffer; a 5-block trainer (random-init weights, max_batch 512) binds the plain view. In the same child:
  - oaz_holdout_mask over the view (share 6 554 / 65 536): one warm-up call, then `--reps` calls, the host's
    monotonic clock around each (the call returns synchronised), ms per call; and oaz_holdout_mask_host once on the
    fetched records;
  - Trainer.evaluate over all records: one warm-up call, `--reps` timed calls, records per second;
  - the training step: `--batches` batches of 512 drawn from the view, a window = `--passes` passes over them, one
    warm-up window, `--reps` timed windows around oaz_trainer_train + sync, ms per step and samples per second;
  - the ratio of the two: the time evaluate spends per 512 records over the time of a step.

(b) The loop (`--loop-games` games per iteration, `--iterations` iterations, `--loop-sims` simulations, 3 blocks,
batch 512, `--epochs` epochs, no pit, random-init weights) with holdout_per_65536 = 6 554: once with
reflect_augment = 1 and merge_duplicates on, once with both off. Per iteration the held-out records and their
metrics before and after the epochs.

usage: python tools/train_eval_bench.py [--out profiles/train_eval_<date>.json] [--sizes 4096,65536] [--reps 5]
                                        [--batches 256] [--passes 4] [--loop-games 2048] [--iterations 4]
                                        [--loop-sims 100] [--epochs 4]"""
from __future__ import annotations

import argparse
import datetime
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import ab

ROOT = Path(__file__).resolve().parents[1]
SEED = 20260101
BATCH, STEP_BLOCKS, NET_BLOCKS, HELD = 512, 5, 3, 6554


def _pkg():
    sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _spread(v):
    return {"each": [round(x, 5) for x in v], "median": statistics.median(v), "min": min(v), "max": max(v)}


def child_eval(args) -> None:
    import numpy as np
    _pkg()
    from onitama_az import _abi, holdout
    from onitama_az.engine import Engine
    from onitama_az.replay import ReplayBuffer
    from onitama_az.trainer import Trainer, choose_batches
    from onitama_az.weights import random_weights

    G = args.games
    with Engine(games=G, sims=400, blocks=NET_BLOCKS, c_puct=5.0, train_noise=1, max_plies=150, evaluator=_abi.EVAL_NN,
                precision=_abi.FP32_SPLIT16, seed=SEED, compact=0, parts=0, sample_capacity=G * 152, fixed_deck=1,
                deck=[0, 1, 2, 3, 4]) as e, ReplayBuffer(capacity=G * 152) as buf, \
            Trainer(blocks=STEP_BLOCKS, max_batch=BATCH) as tr:
        e.load_weights(random_weights(0, NET_BLOCKS))
        t_play, _ = _ms(lambda: e.selfplay_run(G, cap=0))
        buf.append_engine(e, 1)
        ptr, n, _ = buf.view(False)
        tr.set_weights(random_weights(0, STEP_BLOCKS))
        tr.bind_device_samples(ptr, n)
        # the split
        m = holdout.mask((ptr, n), SEED, HELD)
        mask_ms = [_ms(lambda: holdout.mask((ptr, n), SEED, HELD))[0] for _ in range(args.reps)]
        host = buf.fetch(False)[0]
        host_ms, mh = _ms(lambda: holdout.mask(host, SEED, HELD))
        assert np.array_equal(m, mh)
        # the eval-mode pass
        first = tr.evaluate()
        ev_ms = []
        for _ in range(args.reps):
            ms, st = _ms(tr.evaluate)
            assert st == first
            ev_ms.append(ms)
        # the training step on the same records
        idx = choose_batches(np.random.default_rng(0), n, BATCH, args.batches)
        tr.set_batches(idx)
        step_ms = []
        for rep in range(args.reps + 1):  # the first window is the warm-up
            t0 = time.perf_counter()
            for _ in range(args.passes):
                tr.train(0, args.batches)
            tr.sync()
            if rep:
                step_ms.append((time.perf_counter() - t0) * 1e3 / (args.batches * args.passes))
        tr.losses()
    ev, step = statistics.median(ev_ms), statistics.median(step_ms)
    print("RESULT " + json.dumps({
        "games": G, "records": n, "selfplay_ms": t_play, "batch": BATCH, "blocks": STEP_BLOCKS,
        "holdout_mask_ms": _spread(mask_ms), "holdout_mask_host_ms": host_ms, "held_out": int(m.sum()),
        "held_out_share": float(m.mean()), "evaluate_ms": _spread(ev_ms), "evaluate_records_per_s": n / ev * 1e3,
        "step_ms": _spread(step_ms), "step_samples_per_s": BATCH / step * 1e3,
        "evaluate_ms_per_512_records": ev * BATCH / n, "evaluate_over_step": (ev * BATCH / n) / step,
        "evaluation": first.summary()}), flush=True)


def child_loop(args) -> None:
    _pkg()
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train

    on = args.case == "on"
    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=NET_BLOCKS),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=args.loop_sims, train=True),
                     iterations=args.iterations, training_epochs=args.epochs, train_batch_size=BATCH,
                     self_play_game_amnt=args.loop_games, save_checkpoint=10 ** 6, evaluation_checkpoint=10 ** 6,
                     holdout_per_65536=HELD, reflect_augment=1 if on else 0, merge_duplicates=on)
    with tempfile.TemporaryDirectory() as tmp:
        ms, st = _ms(lambda: train(cfg, folder=tmp))
    print("RESULT " + json.dumps({
        "reflect_augment": cfg.reflect_augment, "merge_duplicates": cfg.merge_duplicates, "games": args.loop_games,
        "iterations": args.iterations, "sims": args.loop_sims, "epochs": args.epochs, "wall_ms": ms,
        "training_loss": st.loss, "training_value_loss": st.value_loss, "training_policy_loss": st.policy_loss,
        "games_played": st.games_played, "evaluation": st.evaluation}), flush=True)


def child_cmd(args, mode, games=None, case=None) -> list:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", mode, "--reps", str(args.reps), "--batches",
           str(args.batches), "--passes", str(args.passes), "--loop-games", str(args.loop_games), "--iterations",
           str(args.iterations), "--loop-sims", str(args.loop_sims), "--epochs", str(args.epochs)]
    return cmd + (["--games", str(games)] if games else []) + (["--case", case] if case else [])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=256)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--loop-games", type=int, default=2048)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--loop-sims", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--child", default=None, choices=["eval", "loop"], help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=4096, help=argparse.SUPPRESS)
    ap.add_argument("--case", default="off", choices=["on", "off"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"eval": child_eval, "loop": child_loop}[args.child](args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"train_eval_{date}.json")
    doc = {"tool": "tools/train_eval_bench.py", "date": date,
           "method": "per measurement a child process. throughput: one self-play iteration in a ReplayBuffer, a 5-block "
                     "trainer bound to the plain view; evaluate over all records and oaz_holdout_mask, one warm-up call "
                     "then `reps` timed calls each; the training step over `batches` batches of 512 of the same records, "
                     "one warm-up window then `reps` windows of `passes` passes, host clock around oaz_trainer_train + "
                     "sync. loop: holdout_per_65536 = 6554, the held-out records evaluated before and after each "
                     "iteration's epochs",
           "out_of_scope": "playing strength: no game is played with the trained networks",
           "throughput": [], "loop": []}
    run = ab.Run(out, doc)
    for games in [int(x) for x in args.sizes.split(",") if x]:
        res = run.child(f"eval {games}", child_cmd(args, "eval", games=games), 600)[-1]
        print(f"{games} games, {res['records']} records: evaluate {res['evaluate_records_per_s']:.0f} records/s, step "
              f"{res['step_samples_per_s']:.0f} samples/s, ratio {res['evaluate_over_step']:.3f}, mask "
              f"{res['holdout_mask_ms']['median']:.3f} ms", flush=True)
        doc["throughput"].append(res)
        run.save()
    for case in ("off", "on"):
        res = run.child(f"loop {case}", child_cmd(args, "loop", case=case), 600)[-1]
        for e in res["evaluation"]:
            print(f"loop {case} iteration {e['iteration']}: {e['records']} held out, value_mse "
                  f"{e['before']['value_mse']:.4f} -> {e['after']['value_mse']:.4f}, policy_kl "
                  f"{e['before']['policy_kl']:.4f} -> {e['after']['policy_kl']:.4f}, top1 "
                  f"{e['before']['top1_rate']:.3f} -> {e['after']['top1_rate']:.3f}", flush=True)
        doc["loop"].append(res)
        run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
