"""GPU: the left-right reflection (include/onitama_az.h, "left-right reflection") on the device.

k_reflect_samples against the host entry and the numpy restatement (reflect_util); the GPU rules commute with the
reflection; a trainer whose index entries carry reflect flags equals, bit for bit, a trainer on the buffer
[S, reflected S] with plain indices, and stays within the project's bars of the float64 restatement
(oracle/train_ref.py) fed the reflected planes and pi; the flag check; the loop with LoopConfig.reflect_augment.

Shapes: 1 residual block; batch 16 (the smallest) and 48 (k_gather's last workgroup partly filled: 76 B threads
in workgroups of 256); record counts either side of one wave (63, 64, 65) and with a ragged tail (1000).
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import reflect_util as ru
from onitama_az import _abi
from onitama_az import game
from onitama_az.trainer import Trainer
from onitama_az.weights import named_from_blob
from train_util import HYPER, _batch, _close_grads, _close_params, _weights

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))

pytestmark = pytest.mark.gpu

N_PLAY, SEED = 2000, 20261022


@pytest.fixture(scope="module")
def play(orc):
    return ru.random_play(orc, N_PLAY, SEED)


# ---- oaz_reflect_samples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_reflect_samples_kernel_equals_host_and_restatement(lib, play, n):
    samples = ru.random_samples(play, n, seed=100 + n)
    samples["state"]["pad"] = np.random.default_rng(n).integers(0, 256, (n, 2))
    ref = ru.reflect_samples(samples)
    host = np.zeros_like(samples)
    assert lib.oaz_reflect_samples_host(_abi.ptr(samples), n, _abi.ptr(host)) == 0
    out = np.full(n * _abi.SAMPLE_DTYPE.itemsize, 0x5A, dtype=np.uint8).view(_abi.SAMPLE_DTYPE)
    _abi.check(lib.oaz_reflect_samples(_abi.ptr(samples), n, _abi.ptr(out)))
    assert out.tobytes() == host.tobytes() == ref.tobytes()
    inplace = samples.copy()
    _abi.check(lib.oaz_reflect_samples(_abi.ptr(inplace), n, _abi.ptr(inplace)))
    assert inplace.tobytes() == ref.tobytes()
    assert game.reflect_samples(out, gpu=True).tobytes() == samples.tobytes()  # twice: the bytes again


# ---- the GPU rules commute with the reflection ---------------------------------------------------------------
def test_gpu_rules_commute_with_the_reflection(play):
    n = len(play.states)
    assert n >= 2000
    ru.assert_both_colours_capture_and_win(play)
    s, rs = np.ascontiguousarray(play.states), ru.reflect_states(play.states)
    rm, ra = ru.reflect_moves(play.moves), ru.reflect_states(play.after)
    masks, rmasks = game.movegen_masks_batch(s), game.movegen_masks_batch(rs)
    want = np.zeros_like(masks)
    for f in range(25):
        want[:, :, ru.R(f)] = ru.reflect_boards(masks[:, :, f])
    assert np.array_equal(rmasks, want) and masks.any()
    moves, counts = game.movegen_batch(s)
    rmoves, rcounts = game.movegen_batch(rs)
    assert np.array_equal(counts, rcounts)
    for i in range(n):  # as sets: the order inside a row of the board differs
        assert ru.move_set(ru.reflect_moves(moves[i, :counts[i]])) == ru.move_set(rmoves[i, :rcounts[i]]), i
    a, b = s.copy(), rs.copy()
    res, rres = game.step_batch(a, play.moves), game.step_batch(b, rm)
    assert np.array_equal(res, rres) and np.array_equal(res, play.results)
    assert a.tobytes() == play.after.tobytes() and b.tobytes() == ra.tobytes()
    for x, rx in ((s, rs), (np.ascontiguousarray(play.after), ra)):
        assert np.array_equal(game.current_state_batch(x), game.current_state_batch(rx))
    assert np.any(game.current_state_batch(ra) != _abi.IN_PROGRESS)
    enc, renc = game.encode_batch(s), game.encode_batch(rs)
    assert np.array_equal(renc, ru.reflect_planes(enc)) and np.any(renc != enc)


# ---- trainer: flags in the gather == the doubled buffer, bit for bit ---------------------------------------------
N_BUF, STEPS = 64, 3


def _flags(pattern, B, seed):
    shape = (STEPS, B)
    if pattern == "none":
        return np.zeros(shape, dtype=np.uint8)
    if pattern == "all":
        return np.ones(shape, dtype=np.uint8)
    if pattern == "alternating":
        return (np.arange(STEPS * B).reshape(shape) % 2).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 2, shape, dtype=np.uint8)  # "random", "both"


def _run(tr, w, idx, flags, via):
    """STEPS steps from weights w; flags None = plain set_batches. The raw blobs and loss tuples."""
    tr.set_weights(w)
    tr.losses()
    if flags is None:
        tr.set_batches(idx)
    else:
        tr.set_batches(idx, flags)
    out = []
    if via == "train":
        tr.train(0, STEPS)
        return [tr.grads().tobytes(), tr.get_weights().tobytes(), tr.losses()]
    for s in range(STEPS):
        tr.backward(s)
        out.append(tr.grads().tobytes())
        tr.apply(1.0)
        out += [tr.get_weights().tobytes(), tr.losses()]
    return out


@pytest.fixture(scope="module")
def buffers(orc):
    samples, _ = _batch(orc, N_BUF, 91)
    return samples, np.concatenate([samples, ru.reflect_samples(samples)]), _weights(91, 1)


@pytest.mark.parametrize("via", ["backward", "train"])
@pytest.mark.parametrize("B", [16, 48])
def test_trainer_flags_equal_the_doubled_buffer(buffers, B, via):
    samples, doubled, w = buffers
    rng = np.random.default_rng(B)
    with Trainer(blocks=1, max_batch=B) as ta, Trainer(blocks=1, max_batch=B) as tb:
        ta.load_samples(samples)
        tb.load_samples(doubled)
        seen = set()
        for pattern in ("none", "all", "alternating", "random", "both"):
            idx = np.stack([rng.choice(N_BUF, size=B, replace=False) for _ in range(STEPS)]).astype(np.int32)
            flags = _flags(pattern, B, seed=B + 1)
            if pattern == "both":  # one sample flagged and unflagged in one batch
                idx[:, 1] = idx[:, 0]
                flags[:, 0], flags[:, 1] = 0, 1
            a = _run(ta, w, idx, flags, via)
            b = _run(tb, w, idx + N_BUF * flags.astype(np.int32), None, via)
            assert a == b, pattern
            plain = _run(ta, w, idx, None, via)
            assert (plain == a) == (pattern == "none"), pattern  # flags do change the step; none is set_batches
            seen.add(a[0])
        assert len(seen) == 5


def test_trainer_flags_on_bound_device_samples(buffers):
    """bind_device_samples instead of load_samples: the records in a device buffer of the test's own (the HIP
    runtime the library brought into the process), which the steps only read."""
    samples, doubled, w = buffers
    B = 16
    idx = np.stack([np.random.default_rng(s).choice(N_BUF, size=B, replace=False) for s in range(STEPS)]).astype(np.int32)
    flags = _flags("random", B, seed=7)
    _abi.load()
    hip = C.CDLL(None)  # libamdhip64, loaded with libonitama_az.so (RTLD_GLOBAL)
    for fn in (hip.hipMalloc, hip.hipMemcpy, hip.hipFree):
        fn.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    with Trainer(blocks=1, max_batch=B) as ta, Trainer(blocks=1, max_batch=B) as tb:
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), samples.nbytes) == 0 and dev.value
        try:
            assert hip.hipMemcpy(dev, _abi.ptr(samples), samples.nbytes, 1) == 0  # host to device, synchronous
            ta.bind_device_samples(dev.value, len(samples))
            tb.load_samples(doubled)
            a = _run(ta, w, idx, flags, "backward")
            assert a == _run(tb, w, idx + N_BUF * flags.astype(np.int32), None, "backward")
            back = np.zeros_like(samples)
            assert hip.hipMemcpy(_abi.ptr(back), dev, samples.nbytes, 2) == 0  # device to host
            assert back.tobytes() == samples.tobytes()  # bound samples are only read
        finally:
            ta.sync()
            hip.hipFree(dev)


def test_trainer_flags_against_float64(orc):
    """B = 16, 1 block, 2 steps, random flags: train_ref.train_step (float64) is fed orc.encode of the
    restatement-reflected states and the restatement-reflected pi where the flag is set; gradients, losses and
    parameters within the project's bars (train_util)."""
    from train_ref import train_step
    B, steps, blocks, seed = 16, 2, 1, 93
    samples, planes = _batch(orc, B * steps, seed)
    rsamples = ru.reflect_samples(samples)
    rplanes = np.stack([orc.encode(np.ascontiguousarray(rsamples["state"])[i]) for i in range(len(samples))])
    idx = np.arange(B * steps, dtype=np.int32).reshape(steps, B)[:, ::-1].copy()
    flags = np.random.default_rng(seed).integers(0, 2, idx.shape, dtype=np.uint8)
    assert flags.any() and not flags.all() and np.any(rplanes != planes)
    w = _weights(seed, blocks)
    named, bufs = named_from_blob(w, blocks), None
    ref_kw = dict(lr=HYPER["learning_rate"], momentum=HYPER["momentum"], wd=HYPER["weight_decay"], broadcast=True,
                  bn_momentum=HYPER["bn_momentum"], bn_eps=HYPER["bn_eps"], grad_scale=1.0)
    with Trainer(blocks=blocks, max_batch=B, **HYPER) as tr:
        tr.set_weights(w)
        tr.load_samples(samples)
        tr.set_batches(idx, flags)
        for s in range(steps):
            rows, f = idx[s], flags[s].astype(bool)
            x = np.where(f[:, None, None, None], rplanes[rows], planes[rows])
            pi = np.where(f[:, None], rsamples["pi"][rows], samples["pi"][rows])
            named, grads, lv, lp, bufs = train_step(named, x, pi, samples["z"][rows], blocks, bufs=bufs, **ref_kw)
            tr.backward(s)
            _close_grads(named_from_blob(tr.grads(), blocks), grads)
            tr.apply(1.0)
            v, p, k = tr.losses()
            print(f"step {s}: value loss {v} / {lv}, policy loss {p} / {lp}")
            assert k == 1 and abs(v - lv) <= 1e-5 * abs(lv) + 1e-7 and abs(p - lp) <= 1e-5 * abs(lp) + 1e-7
            _close_params(named_from_blob(tr.get_weights(), blocks), named)


def test_bad_flag_is_rejected_and_leaves_the_batches(lib, buffers):
    samples, _, w = buffers
    B = 16
    idx = np.arange(B, dtype=np.int32).reshape(1, B)
    flags = np.zeros((1, B), dtype=np.uint8)
    flags[0, 3] = 1
    with Trainer(blocks=1, max_batch=B) as tr:
        tr.set_weights(w)
        tr.load_samples(samples)
        tr.set_batches(idx, flags)
        tr.backward(0)
        before = tr.grads().tobytes()
        bad = flags.copy()
        bad[0, B - 1] = 2
        other = idx[:, ::-1].copy()
        assert lib.oaz_trainer_set_batches_reflect(tr._h, _abi.ptr(other), _abi.ptr(bad), 1, B) == _abi.ERR_ARG
        with pytest.raises(_abi.OazError):
            tr.set_batches(other, bad)
        tr.backward(0)
        assert tr.grads().tobytes() == before
        tr.set_batches(idx)  # and the flags do matter
        tr.backward(0)
        assert tr.grads().tobytes() != before


# ---- the loop ---------------------------------------------------------------------------------------------
def test_loop_with_reflect_augment(tmp_path):
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train

    def run(tag, **kw):
        cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=1),
                         mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=8, train=True),
                         iterations=1, training_epochs=2, train_batch_size=16, self_play_game_amnt=16,
                         save_checkpoint=99, evaluation_checkpoint=99, max_plies=20, **kw)
        got = []
        st = train(cfg, folder=str(tmp_path / tag), on_iteration=lambda it, new, best: got.append(new.copy()))
        assert st.iteration == [1] and np.isfinite(st.loss[0]) and len(got) == 1
        return got[0].tobytes(), st.games_played[0]

    (a, ga), (b, _), (off, g0), (default, _) = (run("a", reflect_augment=1), run("b", reflect_augment=1),
                                                run("off", reflect_augment=0), run("default"))
    assert a == b and a != off and off == default
    n = ga["positions_retrieved"]
    assert ga["positions_trained"] == 2 * (n // 16) * 16 and "positions_trained" not in g0
    (two, g2) = run("two", reflect_augment=2)
    assert g2["positions_trained"] == 2 * (2 * n // 16) * 16 and two not in (a, off)
