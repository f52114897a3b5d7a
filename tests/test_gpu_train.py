"""GPU: the training step (csrc/oaz_train.hip through oaz_trainer_*) against the float64 restatement
(oracle/train_ref.py) at the batch, depth and data edges, and the trainer ABI paths beside them.

Every case steps a Trainer and train_ref.train_step on the same data (train_util._run_steps) at the
project's bars: gradients 2e-4 x max|g| + 1e-7, losses 1e-5 relative, parameters 1e-6 + 1e-5 relative.
Two groups (16 blocks, shifted channels) take the fp32 yardstick of train_util instead: per tensor the
larger of the project's bar and 4 x the float32 restatement's own error on the same inputs.

Shapes are the smallest that reach the code named in each docstring (conv workgroups of 32 rows, the
weight gradient's 32-row prefetch step over B/2 rows, the 64-partial unrolled loop of the BN
finalisation).
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from onitama_az import _abi
from onitama_az.engine import Engine
from onitama_az.trainer import Trainer
from onitama_az.weights import blob_from_named, canonical_layout, named_from_blob, read_ot
from train_util import _batch, _run_steps, _weights

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))

pytestmark = pytest.mark.gpu


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a.grads + a.weights, b.grads + b.weights)) and \
        len(a.grads) == len(b.grads) and len(a.weights) == len(b.weights) and a.losses == b.losses


# ---- batch edges -----------------------------------------------------------------------------------
_EDGE = {}


def _edge(orc, B, trainer=None):
    """One step at blocks 1, batch B, in a trainer with max_batch 128; the fresh-trainer result is
    computed once per B and shared."""
    if trainer is not None:
        return _run_steps(orc, blocks=1, B=B, steps=1, seed=30 + B, trainer=trainer)
    if B not in _EDGE:
        _EDGE[B] = _run_steps(orc, blocks=1, B=B, steps=1, seed=30 + B, max_batch=128)
    return _EDGE[B]


@pytest.mark.parametrize("B", [16, 48, 80, 112])
def test_batch_below_max_batch(orc, B):
    """Batches smaller than the buffers' max_batch = 128. B = 48: a conv workgroup (32 rows) half empty
    beside a full one, and 50 conv partials, so the BN finalisation runs its 4-way unrolled loop and its
    tail in one launch; B = 80: 40 rows per weight-gradient split, a remainder behind the 32-row
    prefetch step; B = 112: 3.5 conv workgroups per square; B = 16: one half-empty workgroup."""
    _edge(orc, B)


def test_batch_changes_on_a_live_trainer(orc):
    """One trainer takes B = 128, then 16, then 80 (set_batches, fresh set_weights before each): every
    result equals the same case on a fresh trainer bit for bit, so no partial sum or statistic left
    over from the larger batch is read."""
    with Trainer(blocks=1, max_batch=128) as tr:
        for B in (128, 16, 80):
            assert _same(_edge(orc, B, trainer=tr), _edge(orc, B)), B


# ---- depth edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [0, 5, 16])
def test_depth_edges(orc, lib, blocks):
    """blocks = 0 (one conv: the trunk-backward loop ends in its first pass), 5 (the config's default)
    and 16 (the largest accepted; the conv / BN segment tables full), B = 48, one step. 16 blocks takes
    the fp32 yardstick: 33 convs deep, the project's bars may be out of reach of any fp32 code."""
    out = _run_steps(orc, blocks=blocks, B=48, steps=1, seed=40 + blocks, yardstick=blocks == 16)
    assert len(out.weights[0]) == lib.oaz_weight_count(blocks, 64, 21)
    if blocks == 0:  # an untouched gradient buffer must not pass as "close to a small gradient"
        got = named_from_blob(out.grads[0], blocks)
        for k in out.ref_grads[0]:
            assert np.any(got[k] != 0.0), k


# ---- oaz_trainer_train, determinism ----------------------------------------------------------------
def test_train_three_steps_equals_backward_apply(orc):
    """oaz_trainer_train(0, 3) at 2 blocks, B = 32: parameters, last gradients and the summed losses
    match three restatement steps (k = 3), bit-identical to a twin doing backward(b); apply(1.0) three
    times; losses() accumulates and clears."""
    with Trainer(blocks=2, max_batch=32) as tr:
        a = _run_steps(orc, blocks=2, B=32, steps=3, seed=51, via="train", trainer=tr)
        assert a.losses[-1][2] == 3
        assert tr.losses() == (0.0, 0.0, 0)
    b = _run_steps(orc, blocks=2, B=32, steps=3, seed=51)
    assert a.grads[-1].tobytes() == b.grads[-1].tobytes() and a.weights[-1].tobytes() == b.weights[-1].tobytes()
    assert abs(a.losses[-1][0] - sum(x[0] for x in b.losses)) <= 1e-12  # double sums of the same fp32 terms
    assert abs(a.losses[-1][1] - sum(x[1] for x in b.losses)) <= 1e-12


def test_steps_are_deterministic_and_set_weights_resets_momentum(orc):
    """Fixed-order reductions: the same two steps on two trainers, and twice on one trainer after
    set_weights, give bit-equal gradients and weights. The rerun is also the momentum-reset check:
    with the first run's momentum buffers kept, its weights would differ."""
    kw = dict(blocks=2, B=48, steps=2, seed=52)
    a = _run_steps(orc, **kw)
    with Trainer(blocks=2, max_batch=48) as tr:
        b = _run_steps(orc, trainer=tr, **kw)
        c = _run_steps(orc, trainer=tr, **kw)
    assert _same(a, b) and _same(b, c)


# ---- loss data -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_data(orc, kind):
    B = 16
    samples, planes = _batch(orc, 200 if kind == "repeat_gather" else B, 60)
    idx = None
    pi = samples["pi"].astype(np.float64)
    if kind == "row_sums":  # dl = (p * sum(pi) - pi) / 25B: p - pi would pass normalised rows only
        scale = np.ones(B)
        scale[0::3], scale[1::3] = 0.5, 2.0
        pi *= scale[:, None]
        assert sorted(set(np.round(pi.sum(1), 3))) == [0.5, 1.0, 2.0]
    elif kind == "zero_rows":
        pi[[0, 7, 15]] = 0.0
    elif kind == "one_hot":
        hot = np.argmax(pi, 1)
        pi[:] = 0.0
        pi[np.arange(B), hot] = 1.0
    elif kind == "z_plus_one":
        samples["z"] = 1.0
    elif kind == "repeat_gather":
        idx = np.random.default_rng(60).integers(0, 200, (1, B)).astype(np.int32)
        idx[0, 3] = idx[0, 9] = idx[0, 0]
    samples["pi"] = pi.astype(np.float32)
    return samples, planes, idx


@pytest.mark.parametrize("broadcast", [True, False])
@pytest.mark.parametrize("kind", ["row_sums", "zero_rows", "one_hot", "z_plus_one", "repeat_gather"])
def test_loss_data_edges(orc, kind, broadcast):
    """blocks 1, B = 16: pi rows summing to 0.5 / 2 / 1, all-zero rows (the t != 0 guard on log p, the
    sum(pi) = 0 gradient), one-hot rows, z all +1, and a batch gathered with repeats in random order
    from a 200-sample buffer. The restatement takes pi as given and is the specification: its float64
    losses and gradients are finite here (log(p) * 0 = 0 for finite p), asserted below."""
    samples, planes, idx = _loss_data(orc, kind)
    out = _run_steps(orc, blocks=1, B=16, steps=1, broadcast=broadcast, seed=60, samples=samples, planes=planes,
                     idx=idx)
    assert np.all(np.isfinite(out.ref_losses[0])) and all(np.all(np.isfinite(g)) for g in out.ref_grads[0].values())


def test_real_selfplay_samples(orc):
    """64 samples of hash-evaluator self-play (late-game positions, visit-count pi with exact zeros,
    real z), one step at 2 blocks, B = 64; the restatement's planes come from the oracle's encoder."""
    with Engine(games=64, sims=16, c_puct=5.0, train_noise=1, evaluator=_abi.EVAL_HASH, blocks=0, max_plies=40,
                seed=77, fixed_deck=0) as e:
        e.selfplay_reset()
        e.selfplay_step(40)
        n = int(e.selfplay_stats().samples_ready)
        assert n >= 64
        smp = e.samples_fetch(n)
    samples = np.ascontiguousarray(smp[np.linspace(0, n - 1, 64).astype(np.int64)])  # every phase of the games
    assert (samples["pi"] == 0.0).any() and np.abs(samples["z"]).max() == 1.0
    planes = np.stack([orc.encode(samples["state"][i]) for i in range(64)])
    _run_steps(orc, blocks=2, B=64, steps=1, seed=61, samples=samples, planes=planes)


# ---- hyperparameters -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain_sgd", "bn_knobs", "grad_scale"])
def test_hyperparameters(orc, case):
    """blocks 1, B = 16, two steps: momentum 0 / weight decay 0 / lr 0.1; bn_momentum 0.3 / bn_eps 1e-3;
    apply(0.5) against the restatement's grad_scale = 0.5."""
    kw = {"plain_sgd": dict(hyper=dict(momentum=0.0, weight_decay=0.0, learning_rate=0.1)),
          "bn_knobs": dict(hyper=dict(bn_momentum=0.3, bn_eps=1e-3)),
          "grad_scale": dict(grad_scale=0.5)}[case]
    _run_steps(orc, blocks=1, B=16, steps=2, seed=70, **kw)


# ---- BN statistics exchange, device samples --------------------------------------------------------
def test_bn_stats_pack_unpack(orc, lib):
    """After one step, bn_stats_pack equals the running statistics of get_weights() in the documented
    order (per conv layer mean[64] var[64], the value head's 1 + 1, the policy head's 2 + 2);
    unpack(buf, 0.5) halves exactly those entries and leaves every other parameter bit-equal."""
    blocks = 2
    with Trainer(blocks=blocks, max_batch=16) as tr:
        _run_steps(orc, blocks=blocks, B=16, steps=1, seed=80, trainer=tr)
        w = tr.get_weights()
        running = np.zeros(len(w), dtype=bool)
        off = 0
        for name, shape in canonical_layout(blocks):
            n = int(np.prod(shape))
            running[off:off + n] = name.endswith(("running_mean", "running_var"))
            off += n
        assert running.sum() == lib.oaz_trainer_bn_stats_count(blocks) == (1 + 2 * blocks) * 128 + 6
        buf = torch.zeros(int(running.sum()), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _abi.check(lib.oaz_trainer_bn_stats_pack(tr._h, C.c_void_p(buf.data_ptr())))
        tr.sync()
        named = named_from_blob(w, blocks)
        layers = ["bn1"] + [f"resnet_{i}|resnet_small_block{j}|small_block_bn" for i in range(blocks) for j in (1, 2)]
        layers += ["vh_bn", "policy_bn"]
        doc = np.concatenate([named[f"{bn}|{f}"] for bn in layers for f in ("running_mean", "running_var")])
        assert buf.cpu().numpy().tobytes() == doc.tobytes() == w[running].tobytes()
        _abi.check(lib.oaz_trainer_bn_stats_unpack(tr._h, C.c_void_p(buf.data_ptr()), C.c_float(0.5)))
        tr.sync()
        w2 = tr.get_weights()
    assert w2[~running].tobytes() == w[~running].tobytes()
    assert w2[running].tobytes() == (np.float32(0.5) * w[running]).tobytes() and np.all(w[running] != 0.0)


def test_bind_device_samples_equals_load_samples(orc):
    """The sample bytes in a torch uint8 device tensor (oaz_trainer_bind_device_samples) give bit-equal
    gradients to load_samples."""
    samples, _ = _batch(orc, 48, 81)
    idx = np.random.default_rng(81).permutation(48).astype(np.int32)[:32].reshape(1, 32)
    w = _weights(81, 1)
    got = []
    for bind in (False, True):
        with Trainer(blocks=1, max_batch=32) as tr:
            tr.set_weights(w)
            if bind:
                dev = torch.from_numpy(np.frombuffer(samples.tobytes(), dtype=np.uint8).copy()).cuda()
                torch.cuda.synchronize()
                tr.bind_device_samples(dev.data_ptr(), len(samples))
            else:
                tr.load_samples(samples)
            tr.set_batches(idx)
            tr.backward(0)
            got.append(tr.grads())
    assert np.any(got[0] != 0.0) and got[0].tobytes() == got[1].tobytes()


# ---- trainer to engine -----------------------------------------------------------------------------
def test_trained_weights_evaluate_in_the_engine(orc, tmp_path):
    """Two steps at 2 blocks, B = 32; the weights the trainer hands back (running statistics with the
    unbiased variance, conv weights as k_sgd left them) load into the inference kernels: nn_forward on
    the batch's 64 positions matches train_ref.forward(train=False) in float64 on the same blob within
    1e-4 (exact-fp32 kernel) and 1e-5 (fp16x3 split), the project's bars for those kernels, without
    fp16-range fallback; save_ot -> read_ot returns the blob bit-equal."""
    from train_ref import forward
    blocks = 2
    samples, planes = _batch(orc, 64, 90)
    with Trainer(blocks=blocks, max_batch=32) as tr:
        _run_steps(orc, blocks=blocks, B=32, steps=2, seed=90, samples=samples, planes=planes, trainer=tr)
        w = tr.get_weights()
        tr.save_ot(str(tmp_path / "trained.ot"))
    assert blob_from_named(read_ot(str(tmp_path / "trained.ot")), blocks).tobytes() == w.tobytes()
    with torch.no_grad():
        p, v = forward(named_from_blob(w, blocks), planes, blocks, train=False, dtype=np.float64)
    p, v = p.numpy().reshape(-1, 2, 25), v.numpy().reshape(-1)
    for prec, tol in ((_abi.FP32, 1e-4), (_abi.FP32_SPLIT16, 1e-5)):
        with Engine(games=64, sims=1, blocks=blocks, evaluator=_abi.EVAL_NN, precision=prec) as e:
            e.load_weights(w)
            gp, gv = e.nn_forward(samples["state"])
            assert e.nn_fallbacks() == 0
        dp, dv = float(np.abs(gp - p).max()), float(np.abs(gv - v).max())
        print(f"precision {prec}: max |dp| {dp:.2e}, |dv| {dv:.2e}")
        assert dp < tol and dv < tol, (prec, dp, dv)


# ---- BN statistics under cancellation ------------------------------------------------------------------
def _shifted_weights(planes, seed, blocks):
    """_weights with the first conv's bias set to 8 x the per-channel std of its bias-free output on
    `planes`, signs alternating: every channel's pre-BN |mean| / std is about 8."""
    import torch.nn.functional as F
    w = _weights(seed, blocks).copy()
    named = named_from_blob(w, blocks)  # views into w
    z = F.conv2d(torch.tensor(planes, dtype=torch.float64),
                 torch.tensor(named["conv_init_1|weight"], dtype=torch.float64), None, padding=1)
    std = z.transpose(0, 1).flatten(1).std(1, unbiased=False).numpy()
    named["conv_init_1|bias"][:] = 8.0 * std * np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    zb = z + torch.tensor(named["conv_init_1|bias"], dtype=torch.float64).reshape(1, 64, 1, 1)
    ratio = (zb.transpose(0, 1).flatten(1).mean(1).abs() / torch.tensor(std)).numpy()
    return w, ratio


def test_bn_statistics_with_shifted_channels(orc):
    """blocks 1, B = 48: the batch variance is E[x^2] - mean^2 over fp32 partial sums, which cancels when
    a channel's |mean| is large against its std. Here the first conv's bias puts every channel at
    |mean| / std of about 8. That is roughly five times the 1.72 the trained fixtures reach
    (tests/golden/weights_*_trained.npy, whose pre-BN conv biases are about 1e-8): headroom, not a
    workload the product sees. fp32 yardstick (module docstring): the float32 restatement's own error on
    the same inputs sets the bar where it exceeds the project's."""
    samples, planes = _batch(orc, 48, 95)
    w, ratio = _shifted_weights(planes, 95, 1)
    print(f"pre-BN |mean| / std over the 64 channels: {ratio.min():.2f} .. {ratio.max():.2f}")
    assert ratio.min() > 4.0  # well past the fixtures' 1.72 in every channel
    idx = np.arange(48, dtype=np.int32).reshape(1, 48)
    _run_steps(orc, blocks=1, B=48, steps=1, seed=95, samples=samples, planes=planes, idx=idx, weights=w,
               yardstick=True)
