"""Shared helpers of the training-step tests (tests/test_train.py, tests/test_gpu_train.py): seeded
batches and weights, the project's bars, and the driver that steps a Trainer beside the float64
restatement (oracle/train_ref.py).

Bars (fp32 GPU vs fp64 CPU): gradients within 2e-4 x the tensor's max |g| (+1e-7), losses within 1e-5
relative, parameters / running stats within 1e-6 + 1e-5 relative after the step. Where a case may be out
of reach of any fp32 code at those bars (`yardstick=True`), the bar per tensor is the larger of the
project's and 4 x the float32 restatement's own error against float64 on the same inputs (the factor
tests/test_gpu.py::test_nn_split16_error_at_fp32_level grants one fp32 path against another); it never
comes from the kernel's output.
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from conftest import random_positions
from onitama_az import _abi
from onitama_az.weights import canonical_layout, named_from_blob, random_weights

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))

YARD = 4.0  # fp32 yardstick factor


def _batch(orc, n, seed):
    rng = np.random.default_rng(seed)
    states = random_positions(orc, n, seed=seed)
    samples = np.zeros(n, dtype=_abi.SAMPLE_DTYPE)
    samples["state"] = states
    pi = rng.random((n, 50)) * (rng.random((n, 50)) < 0.3)
    pi[:, 0] += 1e-3  # never an all-zero row
    samples["pi"] = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    samples["z"] = rng.integers(-1, 2, n).astype(np.float32)
    planes = np.stack([orc.encode(states[i]) for i in range(n)])
    return samples, planes


def _weights(seed, blocks):
    """Random init with non-trivial BN affine/running statistics."""
    rng = np.random.default_rng(seed)
    w = random_weights(seed, blocks).copy()
    off = 0
    for name, shape in canonical_layout(blocks):
        n = int(np.prod(shape))
        if name.endswith("running_var"):
            w[off:off + n] = rng.uniform(0.5, 2.0, n)
        elif name.endswith("running_mean") or (("bn" in name) and name.endswith("bias")):
            w[off:off + n] = rng.normal(0, 0.1, n)
        elif ("bn" in name) and name.endswith("weight"):
            w[off:off + n] = rng.uniform(0.7, 1.3, n)
        off += n
    return w.astype(np.float32)


def _close_grads(got, ref, yard=None):
    """yard: per-tensor max-abs error of the float32 restatement (fp32 yardstick cases only)."""
    errs = {}
    for k, g in ref.items():
        scale = float(np.abs(g).max())
        errs[k] = (float(np.abs(got[k].reshape(g.shape) - g).max()), scale)
    worst = sorted(errs.items(), key=lambda kv: -kv[1][0] / (2e-4 * kv[1][1] + 1e-7))[:4]  # closest to the bar
    print("gradient errors closest to the bar (err, max|g|):", [(k, f"{e:.2e}", f"{sc:.2e}") for k, (e, sc) in worst])
    if yard is not None:
        r = max(errs, key=lambda k: errs[k][0] / max(yard[k], 1e-30))
        print(f"  worst kernel / float32-restatement gradient error: {r}: {errs[r][0]:.2e} / {yard[r]:.2e}")
    for k, (err, scale) in errs.items():
        if yard is None:
            assert err <= 2e-4 * scale + 1e-7, (k, err, scale)
        else:
            assert err <= max(2e-4 * scale + 1e-7, YARD * yard[k]), (k, err, scale, yard[k])


def _close_params(got, ref, yard=None):
    for k, p in ref.items():
        if yard is None:
            np.testing.assert_allclose(got[k].reshape(p.shape), p, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            err = np.abs(got[k].reshape(p.shape) - p)
            bar = np.maximum(1e-6 + 1e-5 * np.abs(p), YARD * yard[k])
            assert (err <= bar).all(), (k, float(err.max()), yard[k])


def _max_err(a, b):
    return {k: float(np.abs(np.asarray(a[k], dtype=np.float64) - b[k]).max()) for k in b}


HYPER = dict(learning_rate=5e-3, momentum=0.9, weight_decay=1e-4, bn_momentum=0.1, bn_eps=1e-5)


def _run_steps(orc, blocks, B, steps, broadcast=True, seed=1, max_batch=None, idx=None, samples=None, planes=None,
               weights=None, hyper=None, grad_scale=1.0, via="backward", trainer=None, yardstick=False):
    """`steps` steps of a Trainer beside train_ref.train_step (float64) on the same data; asserts the
    bars above after every step (via="backward": backward(s); apply(grad_scale)) or after all of them
    (via="train": one oaz_trainer_train(0, steps); parameters, the last step's gradients and the summed
    losses). Defaults: a trainer of its own with max_batch = B, the _batch / _weights data of `seed`,
    batch s = samples [sB, (s+1)B) reversed, the default hyperparameters.

    max_batch: the trainer's capacity (>= B); idx: [steps, B] int32 index matrix into `samples`;
    samples / planes: the replay buffer and its encoded planes [n, 21, 5, 5]; weights: the start blob;
    hyper: overrides of HYPER, given to the Trainer and the restatement alike; trainer: a live Trainer to
    reuse (fresh set_weights / load_samples / set_batches, left open); yardstick: see the module docstring.
    Returns the raw fp32 blobs grads[s], weights[s] (after step s; via="train": the last only), the
    losses() tuples, and the restatement's ref_grads[s] / ref_losses[s]."""
    from onitama_az.trainer import Trainer
    from train_ref import train_step
    if samples is None:
        samples, planes = _batch(orc, B * steps, seed)
    w = _weights(seed, blocks) if weights is None else weights
    if idx is None:
        idx = np.arange(B * steps, dtype=np.int32).reshape(steps, B)[:, ::-1].copy()  # non-trivial gather
    hp = dict(HYPER, **(hyper or {}))
    ref_kw = dict(lr=hp["learning_rate"], momentum=hp["momentum"], wd=hp["weight_decay"], broadcast=broadcast,
                  bn_momentum=hp["bn_momentum"], bn_eps=hp["bn_eps"], grad_scale=grad_scale)
    named = named_from_blob(w, blocks)
    named32, bufs, bufs32 = named, None, None
    out = SimpleNamespace(grads=[], weights=[], losses=[], ref_grads=[], ref_losses=[])
    tr = trainer if trainer is not None else Trainer(blocks=blocks, max_batch=max_batch or B,
                                                     value_loss_broadcast=broadcast, **hp)
    try:
        tr.set_weights(w)
        if trainer is not None:
            tr.losses()  # a reused trainer starts from cleared accumulators
        tr.load_samples(samples)
        tr.set_batches(idx)
        if via == "train":
            tr.train(0, steps)
        slv = slp = 0.0
        for s in range(steps):
            rows = idx[s]
            data = (planes[rows], samples["pi"][rows], samples["z"][rows], blocks)
            named, grads, lv, lp, bufs = train_step(named, *data, bufs=bufs, **ref_kw)
            out.ref_grads.append(grads)
            out.ref_losses.append((lv, lp))
            gy = py = ly = None
            if yardstick:
                named32, g32, lv32, lp32, bufs32 = train_step(named32, *data, bufs=bufs32, dtype=np.float32, **ref_kw)
                gy, py, ly = _max_err(g32, grads), _max_err(named32, named), (abs(lv32 - lv), abs(lp32 - lp))
            slv, slp = slv + lv, slp + lp
            if via == "train" and s < steps - 1:
                continue
            if via == "backward":
                tr.backward(s)
            out.grads.append(tr.grads())
            _close_grads(named_from_blob(out.grads[-1], blocks), grads, gy)
            if via == "backward":
                tr.apply(grad_scale)
                slv, slp = lv, lp  # losses() clears: this step's alone
            v, p, k = tr.losses()
            out.losses.append((v, p, k))
            assert k == (steps if via == "train" else 1)
            bv, bp = 1e-5 * abs(slv) + 1e-7, 1e-5 * abs(slp) + 1e-7
            if yardstick:
                print(f"  loss errors kernel / float32 restatement: value {abs(v - slv):.2e} / {ly[0]:.2e}, "
                      f"policy {abs(p - slp):.2e} / {ly[1]:.2e}")
                bv, bp = max(bv, YARD * ly[0]), max(bp, YARD * ly[1])
            assert abs(v - slv) <= bv and abs(p - slp) <= bp, (v, slv, p, slp)
            out.weights.append(tr.get_weights())
            got = named_from_blob(out.weights[-1], blocks)
            if yardstick:
                e = _max_err(got, named)
                r = max(e, key=lambda k: e[k] / max(py[k], 1e-30))
                print(f"  worst kernel / float32-restatement parameter error: {r}: {e[r]:.2e} / {py[r]:.2e}")
            _close_params(got, named, py)
    finally:
        if trainer is None:
            tr.close()
    return out
