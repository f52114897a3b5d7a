#!/usr/bin/env python3
"""Digests of the training step, to compare two builds of the library bit for bit: run it once per library
(OAZ_LIB=<path>, default the in-tree product build) and compare the lines. One JSON line per case: the sha256 of
the gradients after the last backward, of the weights, of the packed BN running statistics
(oaz_trainer_bn_stats_pack) and of the losses() tuple (also printed). Seeded data from tests/train_util.py
(_batch, _weights); batch s is samples [sB, (s + 1)B) reversed. A second or two per case.

  case  blocks  B   max_batch  steps
  1     0       16  16         2      backward + apply: 25 conv partials (the reduction's tail only), the
                                      trunk-backward loop ends in its first pass
  2     2       48  64         3      one oaz_trainer_train(0, 3), every third index entry reflected, momentum
                                      0.9: 50 conv partials (the unrolled loop and its tail in one launch)
  3     1       80  128        2      elementwise value loss, apply(0.5): a remainder behind the weight
                                      gradient's prefetch

usage: [OAZ_LIB=...] python tools/train_digest.py [--case N]"""
import argparse
import ctypes as C
import hashlib
import json
import struct
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "onitama-alphazero_amd"), str(ROOT / "tests")]

CASES = {
    1: dict(blocks=0, B=16, max_batch=16, steps=2, via="backward"),
    2: dict(blocks=2, B=48, max_batch=64, steps=3, via="train", reflect_every=3, hyper=dict(momentum=0.9)),
    3: dict(blocks=1, B=80, max_batch=128, steps=2, via="backward", broadcast=False, grad_scale=0.5),
}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(n, orc, lib):
    import torch
    from onitama_az import _abi
    from onitama_az.trainer import Trainer
    from train_util import HYPER, _batch, _weights
    c = CASES[n]
    blocks, B, steps = c["blocks"], c["B"], c["steps"]
    samples, _ = _batch(orc, B * steps, seed=100 + n)
    idx = np.arange(B * steps, dtype=np.int32).reshape(steps, B)[:, ::-1].copy()
    reflect = None
    if "reflect_every" in c:
        reflect = (np.arange(idx.size) % c["reflect_every"] == 0).astype(np.uint8).reshape(idx.shape)
    with Trainer(blocks=blocks, max_batch=c["max_batch"], value_loss_broadcast=c.get("broadcast", True),
                 **dict(HYPER, **c.get("hyper", {}))) as tr:
        tr.set_weights(_weights(100 + n, blocks))
        tr.load_samples(samples)
        tr.set_batches(idx, reflect)
        if c["via"] == "train":
            tr.train(0, steps)
        else:
            for s in range(steps):
                tr.backward(s)
                tr.apply(c.get("grad_scale", 1.0))
        grads, weights, losses = tr.grads(), tr.get_weights(), tr.losses()
        bn = torch.zeros(int(lib.oaz_trainer_bn_stats_count(blocks)), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _abi.check(lib.oaz_trainer_bn_stats_pack(tr._h, C.c_void_p(bn.data_ptr())))
        tr.sync()
        bn = bn.cpu().numpy()
    return {"case": n, "lib": Path(lib._name).name, "grads": _sha(grads), "weights": _sha(weights),
            "bn_stats": _sha(bn), "losses_sha": hashlib.sha256(struct.pack("<ddq", *losses)).hexdigest(),
            "losses": list(losses)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", type=int, choices=sorted(CASES), help="one case (default: all)")
    a = ap.parse_args()
    import oracle_ffi as orc
    from onitama_az import _abi
    orc.load()
    lib = _abi.load()
    for n in [a.case] if a.case else sorted(CASES):
        print(json.dumps(run_case(n, orc, lib)), flush=True)


if __name__ == "__main__":
    main()
