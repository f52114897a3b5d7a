"""GPU: the held-out split's kernel and the trainer's eval-mode pass (oaz_holdout_mask, oaz_trainer_evaluate,
oaz_trainer_predict; include/onitama_az.h, "held-out evaluation") against tests/train_eval_ref.py: the split
restated with Philox written out, the statistics from oracle/train_ref.py's forward(train=False) in float64.

Bars. predict, per tensor: the larger of 1e-5 absolute and 4 x the float32 restatement's own error against
float64 on the same inputs (the yardstick rule of tests/train_util.py; never from the kernel's output).
evaluate's sums: 1e-5 relative + 1e-7 of float64 (the project's loss bar) or 4 x the float32 restatement's
error. Counts: n and decided exact; top1 and sign on the records that are not borderline (float64 top-two p gap
>= 1e-4, float64 |v| >= 1e-4), at most 2 % left out. The engine cross-check: 2e-5 (each side is held to 1e-5 of
float64).

Measured on an MI355X: predict's largest errors 4e-9 on p and 2e-8 on v with the random weights and 1.4e-6 on p
with the trained ones (the float32 restatement: 5e-9, 1.4e-8 and 9e-7); the sums within 5e-5 absolute of float64
where the float32 restatement is within 3e-4; predict against the engine's fp32 forward 2.2e-6.

Shapes: blocks 1 and 3, max_batch 16 and 48 (one and three 16-row tiles, a conv workgroup of two row groups half
empty at 16 and at 48), n either side of a tile and of max_batch (1, 15, 16, 17, 47, 48, 49) and a ragged 101
(three chunks at 48, seven at 16); the mask kernel either side of a wave (63, 64, 65) and over four workgroups.
"""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import replay_ref as rr
import train_eval_ref as ter
from conftest import GOLDEN
from onitama_az import _abi, holdout
from onitama_az.engine import Engine
from onitama_az.replay import ReplayBuffer
from onitama_az.trainer import Trainer
from train_util import YARD, _batch, _weights

pytestmark = pytest.mark.gpu

N = 600
SEED = 20260101


# ---- shared data and references (computed once; do not change the arrays) --------------------------------------
_DATA = {}


def _data(orc):
    if "d" not in _DATA:
        samples, planes = _batch(orc, N, 77)
        samples.setflags(write=False)
        _DATA["d"] = (samples, planes)
    return _DATA["d"]


@lru_cache(maxsize=None)
def _blob(name):
    if name == "trained3":
        return np.load(GOLDEN / "weights_3block_trained.npy", allow_pickle=False), 3
    blocks = int(name[-1])  # "random1", "random3"
    return _weights(5, blocks), blocks


_REF = {}


def _reference(orc, name, idx=None, reflect=None):
    """float64 and float32 restatements of the entries (idx, reflect) on the weights `name`; the whole buffer
    without flags is computed once per weights."""
    key = (name, None if idx is None else tuple(np.asarray(idx).tolist()),
           None if reflect is None else tuple(np.asarray(reflect).tolist()))
    if key not in _REF:
        samples, _ = _data(orc)
        w, blocks = _blob(name)
        rec, planes = ter.entries(orc, samples, idx, reflect)
        p64, v64 = ter.forward_eval(w, blocks, planes, np.float64)
        p32, v32 = ter.forward_eval(w, blocks, planes, np.float32)
        _REF[key] = SimpleNamespace(rec=rec, p64=p64, v64=v64, p32=p32, v32=v32,
                                    s64=ter.stats(p64, v64, rec["pi"], rec["z"]),
                                    s32=ter.stats(p32, v32, rec["pi"], rec["z"]))
    return _REF[key]


def _trainer(orc, name, max_batch):
    w, blocks = _blob(name)
    tr = Trainer(blocks=blocks, max_batch=max_batch)
    tr.set_weights(w)
    tr.load_samples(_data(orc)[0])
    return tr


def _entries(n, seed):
    """A permuted idx with a repeated index and mixed reflect flags."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(N)[:n].astype(np.int32)
    if n > 2:
        idx[n // 2] = idx[0]
        idx[n - 1] = idx[1]
    return idx, rng.integers(0, 2, n).astype(np.uint8)


# ---- the split's kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_holdout_mask_equals_the_host_entry(n):
    s = rr.synthetic(np.random.default_rng(n).integers(0, max(1, n // 2), n), seed=n + 3)
    with ReplayBuffer() as buf:
        buf.append(s, tag=1)
        ptr, k, _ = buf.view(False)
        assert k == n
        for per in (6554, 16384, 65536, 0):
            got = holdout.mask((ptr, n), SEED, per)
            want = holdout.mask(s, SEED, per)
            assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), per
            assert np.array_equal(want, ter.holdout_mask(s, SEED, per))
        assert buf.fetch(False)[0].tobytes() == s.tobytes()  # the records are only read


# ---- predict ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_batch", [("random1", 16), ("random1", 48), ("random3", 16), ("random3", 48),
                                            ("trained3", 48)])
def test_predict_against_float64(orc, name, max_batch):
    with _trainer(orc, name, max_batch) as tr:
        for n in (1, 15, 16, 17, 47, 48, 49, 101):
            idx, flags = _entries(n, seed=n)
            ref = _reference(orc, name, idx, flags)
            p, v = tr.predict(idx, flags)
            assert p.shape == (n, 50) and v.shape == (n,) and p.dtype == v.dtype == np.float32
            ep, ev = float(np.abs(p - ref.p64).max()), float(np.abs(v - ref.v64).max())
            yp, yv = float(np.abs(ref.p32 - ref.p64).max()), float(np.abs(ref.v32 - ref.v64).max())
            print(f"{name} max_batch {max_batch} n {n}: |dp| {ep:.2e} (float32 restatement {yp:.2e}), "
                  f"|dv| {ev:.2e} ({yv:.2e})")
            assert ep <= max(1e-5, YARD * yp) and ev <= max(1e-5, YARD * yv), (n, ep, yp, ev, yv)
            assert np.abs(p.sum(1) - 1).max() < 1e-5
        p_all, v_all = tr.predict()  # idx None: records 0 .. n-1
        ref = _reference(orc, name)
        assert p_all.shape == (N, 50)
        assert np.abs(p_all - ref.p64).max() <= max(1e-5, YARD * np.abs(ref.p32 - ref.p64).max())
        assert np.abs(v_all - ref.v64).max() <= max(1e-5, YARD * np.abs(ref.v32 - ref.v64).max())
        p0, v0 = tr.predict(np.zeros(0, dtype=np.int32))
        assert p0.shape == (0, 50) and v0.shape == (0,)


def test_predict_bits_do_not_depend_on_place_neighbours_or_max_batch(orc):
    with _trainer(orc, "random3", 16) as t16, _trainer(orc, "random3", 48) as t48:
        idx, flags = _entries(101, seed=1)
        pa, va = t16.predict(idx, flags)
        pb, vb = t48.predict(idx, flags)
        assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()  # max_batch 16 against 48
        perm = np.random.default_rng(2).permutation(101)
        pc, vc = t48.predict(idx[perm], flags[perm])  # other places, other neighbours
        assert pc.tobytes() == pa[perm].tobytes() and vc.tobytes() == va[perm].tobytes()
        for k in (0, 17, 50, 100):  # alone, in a chunk of padding
            p1, v1 = t16.predict(idx[k:k + 1], flags[k:k + 1])
            assert p1.tobytes() == pa[k:k + 1].tobytes() and v1.tobytes() == va[k:k + 1].tobytes()
        pr, vr = t48.predict(idx[:33], flags[:33])  # a prefix: the tail of the chunk is padding now
        assert pr.tobytes() == pa[:33].tobytes() and vr.tobytes() == va[:33].tobytes()
        twice = np.array([idx[0], idx[0], idx[7], idx[0]], dtype=np.int32)  # one record several times in a call
        pt, vt = t48.predict(twice, np.array([flags[0], flags[0], flags[7], flags[0]], dtype=np.uint8))
        assert pt[0].tobytes() == pt[1].tobytes() == pt[3].tobytes() == pa[0].tobytes() and vt[3] == va[0]


# ---- evaluate -----------------------------------------------------------------------------------------------
SUMS = ("value_sq", "policy_ce", "target_entropy")


def _sums(e):
    return (e.value_sq_sum, e.policy_ce_sum, e.target_entropy_sum)


@pytest.mark.parametrize("name", ["random1", "random3", "trained3"])
def test_evaluate_sums_and_counts(orc, name):
    full = _reference(orc, name)
    idx, flags = _entries(101, seed=8)
    part = _reference(orc, name, idx, flags)
    with _trainer(orc, name, 16) as t16, _trainer(orc, name, 48) as t48:
        for ref, args in ((full, ()), (part, (idx, flags))):
            e16, e48, again = t16.evaluate(*args), t48.evaluate(*args), t48.evaluate(*args)
            assert e16 == e48 == again  # the same bytes for every max_batch, and from run to run
            for k, got in zip(SUMS, _sums(e16)):
                r64, r32 = getattr(ref.s64, k), getattr(ref.s32, k)
                print(f"{name} {k}: kernel {got!r} float64 {r64!r} |err| {abs(got - r64):.2e} "
                      f"(float32 restatement {abs(r32 - r64):.2e})")
                assert abs(got - r64) <= max(1e-5 * abs(r64) + 1e-7, YARD * abs(r32 - r64)), (k, got, r64, r32)
            assert e16.n == ref.s64.n and e16.decided == ref.s64.decided
        # top1 and sign on the records that are not borderline in float64. The cap on the share left out holds
        # for the two 3-block networks (0 and 2 of 600 on the CPU); the 1-block random network's priors are
        # within 1e-4 of each other on 138 of the 600 records, so its counts are compared on the other 462.
        clear_p = np.nonzero(full.s64.gap >= 1e-4)[0].astype(np.int32)
        clear_v = np.nonzero(full.s64.absv >= 1e-4)[0].astype(np.int32)
        print(f"{name}: left out of top1 {N - len(clear_p)}, of sign {N - len(clear_v)} of {N}")
        if name != "random1":
            assert N - len(clear_p) <= 0.02 * N and N - len(clear_v) <= 0.02 * N
        e = t48.evaluate(clear_p)
        assert e.n == len(clear_p) and e.top1 == int(full.s64.top1_each[clear_p].sum())
        e = t48.evaluate(clear_v)
        assert e.sign == int(full.s64.sign_each[clear_v].sum()) and e.decided == int(full.s64.decided_each[clear_v].sum())
        assert 0 < e.sign < e.decided or name == "trained3"  # (the golden network's value head is constant)
        # the properties are the sums over the counts
        e = t48.evaluate()
        assert e.value_mse == e.value_sq_sum / N and e.policy_loss == e.policy_ce_sum / (25 * N)
        assert abs(e.policy_kl - (full.s64.policy_ce - full.s64.target_entropy) / N) < 1e-5
        z = t48.evaluate(np.zeros(0, dtype=np.int32))
        assert (z.n, z.decided, z.top1, z.sign) == (0, 0, 0, 0) and _sums(z) == (0.0, 0.0, 0.0)


def test_evaluate_crosses_a_tile_of_the_reduction(orc):
    """2,500 entries (three tiles of 1,024 in the fixed-order sum): the sums are those of the 600 records' terms,
    each counted as often as it is drawn, and the same bytes for both max_batch."""
    idx = np.random.default_rng(12).integers(0, N, 2500).astype(np.int32)
    full = _reference(orc, "random1")
    with _trainer(orc, "random1", 16) as t16, _trainer(orc, "random1", 48) as t48:
        e = t48.evaluate(idx)
        assert e == t16.evaluate(idx)
        p, v = full.p64[idx], full.v64[idx]
        s = ter.stats(p, v, full.rec["pi"][idx], full.rec["z"][idx])
        s32 = ter.stats(full.p32[idx], full.v32[idx], full.rec["pi"][idx], full.rec["z"][idx])
        for k, got in zip(SUMS, _sums(e)):
            r64, r32 = getattr(s, k), getattr(s32, k)
            assert abs(got - r64) <= max(1e-5 * abs(r64) + 1e-7, YARD * abs(r32 - r64)), (k, got, r64, r32)
        assert (e.n, e.decided) == (2500, s.decided)


# ---- the pass changes nothing ---------------------------------------------------------------------------------
def test_evaluate_changes_nothing_a_step_reads_or_reports(orc):
    samples, _ = _data(orc)
    w, blocks = _blob("random1")
    idx = np.random.default_rng(4).permutation(N)[:64].astype(np.int32).reshape(4, 16)
    flags = np.random.default_rng(5).integers(0, 2, (4, 16)).astype(np.uint8)
    with Trainer(blocks=blocks, max_batch=16) as a, Trainer(blocks=blocks, max_batch=16) as b:
        for t in (a, b):
            t.set_weights(w)
            t.load_samples(samples)
            t.set_batches(idx, flags)
            t.backward(0)
        ea = a.evaluate()
        a.predict(np.arange(37, dtype=np.int32))
        assert a.grads().tobytes() == b.grads().tobytes()
        assert a.get_weights().tobytes() == b.get_weights().tobytes()  # running statistics included
        for t in (a, b):
            t.apply()
        a.evaluate(np.arange(5, dtype=np.int32), np.ones(5, dtype=np.uint8))
        assert a.get_weights().tobytes() == b.get_weights().tobytes()
        for t in (a, b):
            t.backward(1)
        a.evaluate()
        assert a.losses() == b.losses()  # both steps' sums: the accumulators were not touched
        for t in (a, b):
            t.apply()
            t.train(0, 4)  # the uploaded index and flag matrix is still there, and the momenta are equal
        a.evaluate()
        assert a.get_weights().tobytes() == b.get_weights().tobytes() and a.losses() == b.losses()
        assert a.grads().tobytes() == b.grads().tobytes()
        assert a.evaluate() != ea  # (the weights did move)


# ---- errors -------------------------------------------------------------------------------------------------
def test_errors(orc, lib):
    samples, _ = _data(orc)
    st = _abi.oaz_eval_stats()
    p, v = np.zeros((4, 50), dtype=np.float32), np.zeros(4, dtype=np.float32)
    with Trainer(blocks=1, max_batch=16) as tr:
        h = tr._h
        idx = np.array([0, 1, 2, 3], dtype=np.int32)
        assert lib.oaz_trainer_evaluate(h, _abi.ptr(idx), 4, None, C.byref(st)) == _abi.ERR_STATE  # nothing bound
        assert lib.oaz_trainer_predict(h, _abi.ptr(idx), 4, None, _abi.ptr(p), _abi.ptr(v)) == _abi.ERR_STATE
        with pytest.raises(_abi.OazError):
            tr.evaluate()
        tr.set_weights(_blob("random1")[0])
        tr.load_samples(samples[:10])
        for bad in (10, -1):
            idx[2] = bad
            assert lib.oaz_trainer_evaluate(h, _abi.ptr(idx), 4, None, C.byref(st)) == _abi.ERR_ARG
            assert lib.oaz_trainer_predict(h, _abi.ptr(idx), 4, None, _abi.ptr(p), _abi.ptr(v)) == _abi.ERR_ARG
        assert lib.oaz_trainer_evaluate(h, None, 11, None, C.byref(st)) == _abi.ERR_ARG  # records 0 .. 10 of 10
        idx[2] = 2
        fl = np.array([0, 1, 2, 0], dtype=np.uint8)
        assert lib.oaz_trainer_evaluate(h, _abi.ptr(idx), 4, _abi.ptr(fl), C.byref(st)) == _abi.ERR_ARG
        assert lib.oaz_trainer_evaluate(h, _abi.ptr(idx), 4, None, None) == _abi.ERR_ARG
        assert lib.oaz_trainer_evaluate(None, _abi.ptr(idx), 4, None, C.byref(st)) == _abi.ERR_ARG
        assert lib.oaz_trainer_evaluate(h, None, 10, None, C.byref(st)) == 0 and st.n == 10
        assert tr.evaluate().n == 10


# ---- bound device samples -------------------------------------------------------------------------------------
def test_bound_view_evaluates_as_the_loaded_records(orc):
    samples, _ = _data(orc)
    s = np.concatenate([samples[:300], samples[100:250]])  # duplicates for the merged view
    w, blocks = _blob("random1")
    idx, flags = _entries(101, seed=6)
    idx = (idx % 300).astype(np.int32)
    with ReplayBuffer() as buf, Trainer(blocks=blocks, max_batch=48) as ta, Trainer(blocks=blocks, max_batch=48) as tb:
        buf.append(s, tag=1)
        for merge in (False, True):
            want = buf.fetch(merge)[0].copy()
            ptr, n, _ = buf.view(merge)
            assert n == len(want) == (300 if merge else 450)
            for t in (ta, tb):
                t.set_weights(w)
            ta.bind_device_samples(ptr, n)
            tb.load_samples(want)
            assert ta.evaluate() == tb.evaluate() and ta.evaluate(idx, flags) == tb.evaluate(idx, flags)
            pa, pb = ta.predict(idx, flags), tb.predict(idx, flags)
            assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes()
            m = holdout.mask((ptr, n), SEED, 16384)
            assert np.array_equal(m, holdout.mask(want, SEED, 16384))
            _, held = holdout.split(m)
            assert ta.evaluate(held) == tb.evaluate(held) and ta.evaluate(held).n == int(m.sum())
            assert buf.fetch(merge)[0].tobytes() == want.tobytes()  # bound records are only read


# ---- the engine plays the network the pass evaluates -----------------------------------------------------------
def test_predict_equals_the_engines_forward(orc):
    samples, _ = _data(orc)
    w, blocks = _blob("trained3")
    states = np.ascontiguousarray(samples["state"][:256])
    with Engine(games=256, sims=1, blocks=blocks, evaluator=_abi.EVAL_NN, precision=_abi.FP32) as e:
        e.load_weights(w)
        gp, gv = e.nn_forward(states)
    with _trainer(orc, "trained3", 48) as tr:
        p, v = tr.predict(np.arange(256, dtype=np.int32))
    dp, dv = float(np.abs(gp.reshape(256, 50) - p).max()), float(np.abs(gv - v).max())
    print(f"predict against Engine.nn_forward (OAZ_FP32): max |dp| {dp:.2e}, |dv| {dv:.2e}")
    assert dp <= 2e-5 and dv <= 2e-5, (dp, dv)


# ---- the loop -------------------------------------------------------------------------------------------------
def _loop(tmp_path, tag, record=None, replay=None, **kw):
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train
    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=1),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=16, train=True), iterations=2,
                     training_epochs=2, train_batch_size=16, self_play_game_amnt=32, save_checkpoint=99,
                     evaluation_checkpoint=99, max_plies=20, **kw)
    got = []

    def seen(it, new, best):
        got.append(new.copy())
        if record is not None:
            record(it)

    st = train(cfg, folder=str(tmp_path / tag), on_iteration=seen, replay=replay)
    assert st.iteration == [1, 2] and all(np.isfinite(st.loss)) and len(got) == 2
    return got, st, cfg


@pytest.mark.parametrize("path", ["host", "replay"])
def test_loop_never_trains_on_a_held_out_position(tmp_path, monkeypatch, path):
    """Two tiny iterations with a quarter held out: every batch the trainer is given is recorded (a wrapped
    set_batches), the iteration's records come from the wrapped load_samples or the caller's replay window, and
    the restated rule says which of them are held out."""
    drawn, loaded, per_it = [], [], []
    real_set, real_load = Trainer.set_batches, Trainer.load_samples

    def set_batches(self, idx, reflect=None):
        drawn.append(np.array(idx, dtype=np.int32).reshape(-1))
        return real_set(self, idx, reflect)

    def load_samples(self, samples):
        loaded.append(np.array(samples))
        return real_load(self, samples)

    monkeypatch.setattr(Trainer, "set_batches", set_batches)
    monkeypatch.setattr(Trainer, "load_samples", load_samples)
    kw = dict(holdout_per_65536=16384)
    buf = None
    if path == "replay":
        buf = ReplayBuffer(capacity=100_000, window=2)
        kw.update(replay_iterations=2, merge_duplicates=True, reflect_augment=2)

    def record(it):
        recs = buf.fetch(True)[0].copy() if buf is not None else loaded[-1]
        per_it.append((recs, np.concatenate(drawn) if drawn else np.zeros(0, dtype=np.int32)))
        drawn.clear()

    try:
        _, st, cfg = _loop(tmp_path, path, record=record, replay=buf, **kw)
    finally:
        if buf is not None:
            buf.close()
    assert len(st.evaluation) == 2 and len(per_it) == 2
    seen_sides = {}
    for (recs, idx), ev, gp in zip(per_it, st.evaluation, st.games_played):
        m = ter.holdout_mask(recs, cfg.seed, 16384)
        assert len(idx) > 0 and not m[idx].any()  # no held-out record in any batch
        assert ev["records"] == ev["held_out"] == gp["held_out"] == int(m.sum()) > 0
        assert ev["before"]["n"] == ev["after"]["n"] == int(m.sum())
        assert ev["before"] != ev["after"] and np.isfinite(ev["after"]["value_mse"])
        for rec, f in zip(recs, m):  # a position keeps its side from one iteration to the next
            assert seen_sides.setdefault(rec["state"].tobytes()[:22], int(f)) == int(f)


def test_loop_with_the_options_off_is_the_loop_and_evaluating_alone_trains_the_same(tmp_path):
    (a1, a2), sa, _ = _loop(tmp_path, "a")
    (b1, b2), sb, _ = _loop(tmp_path, "b")
    assert a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes() and sa.loss == sb.loss
    assert sa.evaluation == [] and all("held_out" not in g for g in sa.games_played)
    (c1, c2), sc, _ = _loop(tmp_path, "c", evaluate=True)  # nothing held out: all records evaluated, same training
    assert c1.tobytes() == a1.tobytes() and c2.tobytes() == a2.tobytes() and sc.loss == sa.loss
    assert [e["records"] for e in sc.evaluation] == [g["positions_retrieved"] for g in sc.games_played]
    assert all(e["held_out"] == 0 for e in sc.evaluation)
