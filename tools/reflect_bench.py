#!/usr/bin/env python3
"""The left-right reflection in training (Trainer.set_batches(idx, reflect), train_epochs(reflect=...)): what the
flags cost per SGD step, and how far a network is from reflection symmetry with and without them. Measurement
tool; bench.py is the flagship's and is not touched. What the augmentation is worth in playing strength is not
measured here.

Every measurement runs in a child process of its own under `timeout`, one at a time; the first child
without exit status 0 and a result ends the whole run (tools/ab.py). One child first plays the data: a training
buffer (`--games` self-play games,
3-block random-init network seed 0, `--sims` simulations, root noise) and, from another seed, the fixed positions
the gaps are measured on (the first `--positions` records of as many games).

(a) Step time: batch 512, 5 residual blocks, random-init weights, `--batches` batches of the buffer. A window is
`--passes` passes over the batches (2 048 steps, about 1.5 s: shorter windows measure the clock and the scheduler as
much as the step). Warm-up: one window; then `--reps` timed windows, the host's monotonic clock around the
oaz_trainer_train calls + sync, reported as ms per step (per window, their median, minimum and maximum). Cases:
flags absent (set_batches(idx)), random flags, all flags set. `--parent DIR`: a checkout of the parent commit, built; "flags absent" is then also
measured with DIR's package and library, alternating with this tree's (this tree, parent, this tree, parent), and
accepted when this tree's slower run is no slower than the parent's slower run by more than the parent's two
runs differ from each other.

(b) Reflection gap of a network on the fixed positions s: policy gap = mean over s of max over (k, t) of
|p(s)[k][t] - p(R s)[k][R t]|, value gap = mean over s of |v(s) - v(R s)| (Engine.nn_forward, fp16x3). Networks:
the trained 3-block golden weights, the start weights (3 blocks, random init seed 0), and three networks trained
from those start weights on the buffer (cut to whole batches) for the same number of steps with reflect 0, 1 and 2
(`--epochs` epochs for 0 and 1, half as many for 2, whose epochs are twice as long), with the losses of each epoch.

usage: python tools/reflect_bench.py [--out profiles/reflect_<date>.json] [--parent DIR] [--games 1024] [--sims 64]
                                     [--positions 4096] [--batches 256] [--passes 8] [--reps 5] [--epochs 32]"""
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
BATCH, STEP_BLOCKS, NET_BLOCKS = 512, 5, 3


def _pkg(args):
    sys.path.insert(0, str(Path(args.pkg) if args.pkg else ROOT / "onitama-alphazero_amd"))


def child_data(args) -> None:
    import numpy as np
    _pkg(args)
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.weights import random_weights

    out = {}
    for key, seed, games in (("buffer", 20260101, args.games), ("positions", 20260202, max(64, args.positions // 8))):
        with Engine(games=games, sims=args.sims, blocks=NET_BLOCKS, c_puct=5.0, train_noise=1, max_plies=150,
                    evaluator=_abi.EVAL_NN, precision=_abi.FP32_SPLIT16, seed=seed, sample_capacity=games * 152) as e:
            e.load_weights(random_weights(0, NET_BLOCKS))
            out[key], _ = e.selfplay_run(games, cap=games * 152)
    assert len(out["positions"]) >= args.positions, "too few positions: raise --games"
    np.save(args.data + ".buffer.npy", out["buffer"].view(np.uint8))
    np.save(args.data + ".positions.npy", out["positions"][:args.positions].view(np.uint8))
    print("RESULT " + json.dumps({"buffer_samples": int(len(out["buffer"])), "positions": args.positions,
                                  "games": args.games, "sims": args.sims}), flush=True)


def _load(args, what):
    import numpy as np
    from onitama_az import _abi
    return np.load(f"{args.data}.{what}.npy").view(_abi.SAMPLE_DTYPE).reshape(-1)


def child_step(args) -> None:
    import numpy as np
    _pkg(args)
    from onitama_az.trainer import Trainer, choose_batches
    from onitama_az.weights import random_weights

    samples = _load(args, "buffer")
    idx = choose_batches(np.random.default_rng(0), len(samples), BATCH, args.batches)
    flags = {"absent": None, "random": np.random.default_rng(1).integers(0, 2, idx.shape, dtype=np.uint8),
             "all": np.ones(idx.shape, dtype=np.uint8)}[args.case]
    with Trainer(blocks=STEP_BLOCKS, max_batch=BATCH) as tr:
        tr.set_weights(random_weights(0, STEP_BLOCKS))
        tr.load_samples(samples)
        if flags is None:  # (the parent's set_batches takes no flags)
            tr.set_batches(idx)
        else:
            tr.set_batches(idx, flags)
        ms = []
        for rep in range(args.reps + 1):  # the first window is the warm-up
            t0 = time.perf_counter()
            for _ in range(args.passes):
                tr.train(0, args.batches)
            tr.sync()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3 / (args.batches * args.passes))
        v, p, k = tr.losses()
    print("RESULT " + json.dumps({"case": args.case, "batch": BATCH, "blocks": STEP_BLOCKS, "batches": args.batches,
                                  "passes_per_window": args.passes, "ms_per_step": [round(x, 5) for x in ms],
                                  "median_ms_per_step": statistics.median(ms), "min_ms_per_step": min(ms), "max_ms_per_step": max(ms),
                                  "mean_loss": (v + p) / max(1, k)}), flush=True)


def child_gap(args) -> None:
    import numpy as np
    _pkg(args)
    from onitama_az import _abi
    from onitama_az.engine import Engine
    from onitama_az.game import reflect_samples, reflect_square
    from onitama_az.trainer import Trainer, train_epochs
    from onitama_az.weights import random_weights

    buf, pos = _load(args, "buffer"), _load(args, "positions")
    buf = buf[:len(buf) // BATCH * BATCH]  # whole batches: n // batch and 2 n // batch steps per epoch, exactly 1 : 2
    states = np.ascontiguousarray(pos["state"])
    rstates = np.ascontiguousarray(reflect_samples(pos)["state"])
    perm = np.array([k * 25 + reflect_square(t) for k in range(2) for t in range(25)])
    start = random_weights(0, NET_BLOCKS)

    def gaps(e, w):
        e.load_weights(w)
        (p, v), (rp, rv) = e.nn_forward(states), e.nn_forward(rstates)
        p, rp = p.reshape(-1, 50).astype(np.float64), rp.reshape(-1, 50).astype(np.float64)
        return {"policy_gap": float(np.abs(p - rp[:, perm]).max(1).mean()),
                "value_gap": float(np.abs(v.astype(np.float64) - rv).mean()),
                "mean_max_policy": float(p.max(1).mean()), "mean_abs_value": float(np.abs(v).mean()),
                "value_std": float(v.astype(np.float64).std())}  # (0: a value head that is constant on the positions)

    nets = [("trained 3-block golden weights", np.load(ROOT / "tests" / "golden" / "weights_3block_trained.npy"), None),
            ("start weights (random init, seed 0)", start, None)]
    for mode in (0, 1, 2):
        epochs = args.epochs // 2 if mode == 2 else args.epochs
        with Trainer(blocks=NET_BLOCKS, max_batch=BATCH) as tr:
            tr.set_weights(start)
            hist = train_epochs(tr, buf, epochs=epochs, batch=BATCH, seed=7, reflect=mode)
            nets.append((f"trained from the start weights, reflect {mode}", tr.get_weights(),
                         {"reflect": mode, "epochs": epochs, "steps": sum(h.steps for h in hist),
                          "loss": [h.loss for h in hist], "value_loss": [h.value for h in hist],
                          "policy_loss": [h.policy for h in hist]}))
    out = []
    with Engine(games=len(states), sims=1, blocks=NET_BLOCKS, evaluator=_abi.EVAL_NN, precision=_abi.FP32_SPLIT16) as e:
        for name, w, training in nets:
            out.append(dict({"network": name, "training": training}, **gaps(e, w)))
    print("RESULT " + json.dumps({"positions": int(len(states)), "buffer_samples": int(len(buf)), "batch": BATCH,
                                  "networks": out}), flush=True)


def child_cmd(args, mode, data, case=None, pkg=None) -> list:
    """The command of one measurement's child process."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", mode, "--data", data, "--games", str(args.games),
           "--sims", str(args.sims), "--positions", str(args.positions), "--batches", str(args.batches),
           "--reps", str(args.reps), "--epochs", str(args.epochs), "--passes", str(args.passes)]
    return cmd + (["--case", case] if case else []) + (["--pkg", str(pkg)] if pkg else [])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=256)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=32, help="even")
    ap.add_argument("--child", default=None, choices=["data", "step", "gap"], help=argparse.SUPPRESS)
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--case", default="absent", choices=["absent", "random", "all"], help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"data": child_data, "step": child_step, "gap": child_gap}[args.child](args)
    date = datetime.date.today().isoformat()
    out = Path(args.out or ROOT / "profiles" / f"reflect_{date}.json")
    doc = {"tool": "tools/reflect_bench.py", "date": date,
           "method": "per measurement a child process. data: self-play records (3-block random-init network). step time: "
                     "batch 512, 5 blocks, a window = `passes_per_window` passes over `batches` batches; one warm-up window, "
                     "then `reps` timed windows, host clock around oaz_trainer_train + sync, ms per step. gap: mean over the positions of max |p(s)[k][t] - "
                     "p(Rs)[k][Rt]| and of |v(s) - v(Rs)|; the three trained networks take the same number of steps",
           "out_of_scope": "what the augmentation is worth in playing strength",
           "data": None, "step_time": [], "step_time_parent": [], "absent_against_parent": None, "reflection_gap": None}

    run = ab.Run(out, doc)

    def one(mode, data, case=None, pkg=None):
        what = f"{mode} {case or ''} {'parent' if pkg else 'this tree'}"
        res = run.child(what, child_cmd(args, mode, data, case=case, pkg=pkg), 600)[-1]
        print(f"{what}: {res.get('median_ms_per_step', '')}", flush=True)
        return res

    with tempfile.TemporaryDirectory() as tmp:
        data = str(Path(tmp) / "reflect")
        doc["data"] = one("data", data)
        run.save()
        sides = [(None, "step_time")]
        if args.parent:  # this tree and the parent, alternating
            sides.append((Path(args.parent) / "onitama-alphazero_amd", "step_time_parent"))
        for pkg, key in ab.schedule(sides, 2):
            doc[key].append(one("step", data, case="absent", pkg=pkg))
            run.save()
        if args.parent:  # "flags absent" against the parent, in ms per step
            mine, theirs = ([r["median_ms_per_step"] for r in doc[k]] for k in ("step_time", "step_time_parent"))
            v = ab.spread_verdict(mine, theirs, higher_is_better=False)
            doc["absent_against_parent"] = {
                "this_tree_median_ms_per_step": v["mine"], "parent_median_ms_per_step": v["other"],
                "parent_spread_ms": v["other_spread"], "this_tree_slower_by_ms": v["behind_by"], "accepted": v["accepted"]}
        for case in ("random", "all"):
            doc["step_time"].append(one("step", data, case=case))
            run.save()
        doc["reflection_gap"] = one("gap", data)
    run.save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
