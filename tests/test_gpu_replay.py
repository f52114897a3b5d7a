"""GPU: the device replay buffer (oaz_replay_*, csrc/oaz_replay.hip; include/onitama_az.h, "replay buffer").

The merged view against the numpy restatement (replay_ref) and oaz_replay_merge_host, bit for bit; the plain
view and the window against the restated window; the three appends against each other and against
samples_fetch; a Trainer bound to a view against a Trainer that loaded the same records; the loop's replay path.

Shapes: record counts either side of one wave (63, 64, 65), a ragged 1,000, 4,097 distinct records (one past a
scan tile of 4,096: the second scan level adds a non-zero offset), 20,000 records with a group of 5,000 (78
members per lane of its wave) beside 500 small groups, and 1,000 keys in 1,024 slots (load 0.98: long probe
chains that wrap around the table's end). Records are synthetic except where an engine or a trainer reads them.
"""
import ctypes as C

import numpy as np
import pytest

import replay_ref as rr
from onitama_az import _abi
from onitama_az.engine import Engine
from onitama_az.replay import ReplayBuffer, merge_host
from onitama_az.trainer import Trainer
from train_util import _batch, _weights

pytestmark = pytest.mark.gpu


def _merged_equals(buf, samples, ref=None):
    out, mult = buf.fetch(merge=True)
    ro, rm = rr.merge(samples) if ref is None else ref
    ho, hm = merge_host(samples)
    assert len(out) == len(ro) == len(ho) and np.array_equal(mult, rm) and np.array_equal(hm, rm)
    assert ho.tobytes() == ro.tobytes()
    assert out.tobytes() == ro.tobytes()
    st = buf.stats()
    assert (st.unique, st.max_mult, st.records) == (len(ro), int(rm.max()), len(samples))
    return st


# ---- the merged view ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_merged_view_equals_restatement_and_host(n):
    ids = np.random.default_rng(n).integers(0, max(1, n // 3), n)
    s = rr.synthetic(ids, seed=n + 1)
    with ReplayBuffer() as buf:
        buf.append(s, tag=1)
        st = _merged_equals(buf, s)
        assert st.probes >= n - st.unique  # every record that is not the first of its key compared at least once
        assert set(buf.merge_times()) == set(_abi.REPLAY_PHASES) and all(t >= 0 for t in buf.merge_times().values())
        ptr, k, mptr = buf.view(merge=True)
        assert ptr and mptr and k == st.unique


@pytest.fixture(scope="module")
def big():
    """20,000 records: one group of 5,000 and 500 groups of 2 .. 60, shuffled; the restatement's merge, once."""
    rng = np.random.default_rng(20)
    small = rng.integers(2, 61, 500)
    while small.sum() != 15000:  # move single records between groups until the total fits
        k = rng.integers(0, 500)
        step = 1 if small.sum() < 15000 else -1
        if 2 <= small[k] + step <= 60:
            small[k] += step
    s = rr.synthetic(rr.mixed_ids(np.concatenate([[5000], small]), seed=21), seed=22)
    assert len(s) == 20000
    s.setflags(write=False)
    return s, rr.merge(s)


@pytest.mark.parametrize("slots", [0, 32768])  # auto (65,536), and the smallest power of two above 20,000
def test_one_large_group_among_many_small_ones(big, slots):
    s, ref = big
    with ReplayBuffer(table_slots=slots) as buf:
        buf.append(s)
        st = _merged_equals(buf, s, ref)
        assert (st.unique, st.max_mult) == (501, 5000)


def test_a_table_at_load_098_probes_long_chains_and_wraps():
    s = rr.synthetic(np.arange(1000), seed=30)
    with ReplayBuffer(table_slots=1024) as buf:
        buf.append(s)
        st = _merged_equals(buf, s)
        assert st.unique == 1000 and st.probes > 1000  # collisions were walked, with 24 free slots
        out, _ = buf.fetch(merge=True)
        assert out.tobytes() == s.tobytes()


@pytest.mark.parametrize("slots", [0, 8192])
def test_distinct_records_across_a_scan_tile(slots):
    s = rr.synthetic(np.arange(4097), seed=31)
    with ReplayBuffer(table_slots=slots) as buf:
        buf.append(s)
        out, mult = buf.fetch(merge=True)
        assert out.tobytes() == s.tobytes() and np.all(mult == 1) and len(out) == 4097
        dup = np.concatenate([s, s[4090:]])  # the last group's position lies in the second tile
        buf.append(dup)
        _merged_equals(buf, dup)


@pytest.mark.parametrize("n,slots", [(1000, 512), (1000, 1000), (1024, 1024), (5, 6)])
def test_a_table_that_cannot_hold_the_view_is_refused(lib, n, slots):
    s = rr.synthetic(np.arange(n), seed=32)
    with ReplayBuffer(table_slots=slots) as buf:
        buf.append(s)
        p, m, k = C.c_void_p(), C.c_void_p(), C.c_size_t(77)
        assert lib.oaz_replay_view(buf._h, 1, C.byref(p), C.byref(k), C.byref(m)) == _abi.ERR_ARG
        assert b"table_slots" in lib.oaz_last_error()
        st = buf.stats()
        assert (st.unique, st.probes, st.records) == (0, 0, n) and sum(buf.merge_times().values()) == 0  # nothing ran
        out, mult = buf.fetch(merge=False)
        assert out.tobytes() == s.tobytes() and np.all(mult == 1)


# ---- the plain view and the window --------------------------------------------------------------------------
SIZES = (100, 0, 200, 50, 300)


@pytest.mark.parametrize("capacity", [180_000, 400])
def test_window_of_three(lib, capacity):
    segs = [rr.synthetic(np.random.default_rng(40 + i).integers(0, 50, k), seed=50 + i) for i, k in enumerate(SIZES)]
    with ReplayBuffer(capacity=capacity, window=3) as buf:
        assert buf.view()[1:] == (0, None) and buf.view(merge=True)[1:] == (0, None)  # an empty window
        assert buf.fetch(merge=True)[0].size == 0
        for i, seg in enumerate(segs):
            buf.append(seg, tag=i)
            want = rr.concat(rr.window(segs[:i + 1], 3, capacity))
            out, mult = buf.fetch()
            assert out.tobytes() == want.tobytes() and np.all(mult == 1), i
            st = buf.stats()
            assert st.records == len(want) and st.segments == len(rr.window(segs[:i + 1], 3, capacity))
            assert st.appended == sum(SIZES[:i + 1]) and st.evicted == st.appended - len(want)
        want = rr.concat(rr.window(segs, 3, capacity))
        assert len(want) == (350 if capacity == 400 else 550)
        _merged_equals(buf, want)
        if capacity == 400:  # a segment above the capacity is refused and nothing changes
            before = buf.stats()
            too_many = rr.synthetic(np.arange(401), seed=60)
            assert lib.oaz_replay_append_host(buf._h, _abi.ptr(too_many), 401, 9) == _abi.ERR_CAPACITY
            assert b"401" in lib.oaz_last_error()
            after = buf.stats()
            assert all(getattr(before, f) == getattr(after, f) for f, _ in before._fields_)
            assert buf.fetch()[0].tobytes() == want.tobytes()
            buf.append(too_many[:400], tag=10)  # exactly the capacity: alone in the window
            assert buf.fetch()[0].tobytes() == too_many[:400].tobytes() and buf.stats().segments == 1


# ---- the three appends --------------------------------------------------------------------------------------
def _hip():
    _abi.load()
    hip = C.CDLL(None)  # libamdhip64, loaded with libonitama_az.so (RTLD_GLOBAL)
    for fn in (hip.hipMalloc, hip.hipMemcpy, hip.hipFree):
        fn.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_append_device_equals_append_host():
    a, b = (rr.synthetic(np.random.default_rng(70 + i).integers(0, 40, 300), seed=72 + i) for i in range(2))
    hip = _hip()
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), a.nbytes) == 0 and dev.value
    try:
        with ReplayBuffer(window=2) as h, ReplayBuffer(window=2) as d:
            for seg in (a, b):
                assert hip.hipMemcpy(dev, _abi.ptr(seg), seg.nbytes, 1) == 0  # host to device, synchronous
                h.append(seg)
                d.append_device(dev.value, len(seg))
            for merge in (False, True):
                (ho, hm), (do, dm) = h.fetch(merge), d.fetch(merge)
                assert ho.tobytes() == do.tobytes() and np.array_equal(hm, dm)
            assert h.fetch()[0].tobytes() == np.concatenate([a, b]).tobytes()
    finally:
        hip.hipFree(dev)


def test_append_engine_equals_samples_fetch():
    kw = dict(games=64, sims=8, c_puct=5.0, train_noise=1, evaluator=_abi.EVAL_HASH, blocks=0, max_plies=12, seed=81,
              fixed_deck=0)
    with Engine(**kw) as a, Engine(**kw) as b, ReplayBuffer() as buf:
        for e in (a, b):
            e.selfplay_run(64, cap=0)
        ref = b.samples_fetch(64 * 14)
        assert len(ref) > 0
        assert buf.append_engine(a, tag=1) == len(ref)
        assert a.selfplay_stats().samples_ready == 0
        assert buf.fetch()[0].tobytes() == ref.tobytes()
        _merged_equals(buf, ref)
        assert buf.append_engine(a, tag=2) == 0 and buf.stats().records == 0  # an empty segment ages the window of one


# ---- a trainer on a view ------------------------------------------------------------------------------------
def _steps(tr, w, n, B=16, steps=3):
    idx = np.stack([np.random.default_rng(90 + s).choice(n, size=B, replace=False) for s in range(steps)]).astype(np.int32)
    tr.set_weights(w)
    tr.losses()
    tr.set_batches(idx)
    out = []
    for s in range(steps):
        tr.backward(s)
        tr.apply(1.0)
        out += [tr.get_weights().tobytes(), tr.losses()]
    return out


@pytest.mark.parametrize("merge", [False, True])
def test_trainer_bound_to_a_view_equals_a_trainer_that_loaded_it(orc, merge):
    base, _ = _batch(orc, 40, 95)
    dup = base[np.random.default_rng(96).integers(0, 40, 60)].copy()  # 60 more records on the same 40 positions
    dup["pi"] = np.roll(dup["pi"], 7, axis=1)
    dup["z"] = -dup["z"]
    samples = np.concatenate([base, dup])
    want = rr.merge(samples)[0] if merge else samples
    assert len(want) == (len({rr.key_bytes(r) for r in samples}) if merge else 100) and len(want) <= 100 - 60 * merge
    w = _weights(95, 1)
    with ReplayBuffer() as buf, Trainer(blocks=1, max_batch=16) as ta, Trainer(blocks=1, max_batch=16) as tb:
        buf.append(samples)
        ptr, n, _ = buf.view(merge)
        assert n == len(want)
        ta.bind_device_samples(ptr, n)
        tb.load_samples(want)
        assert _steps(ta, w, n) == _steps(tb, w, n)
        ta.sync()
        assert buf.fetch(merge)[0].tobytes() == want.tobytes()  # bound records are only read


# ---- the loop -----------------------------------------------------------------------------------------------
def _loop(tmp_path, tag, replay=None, on_iteration=None, **kw):
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train
    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=1),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=16, train=True), iterations=2,
                     training_epochs=2, train_batch_size=16, self_play_game_amnt=32, save_checkpoint=99,
                     evaluation_checkpoint=99, max_plies=20, **kw)
    got = []

    def seen(it, new, best):
        got.append(new.copy())
        if on_iteration is not None:
            on_iteration(it)

    st = train(cfg, folder=str(tmp_path / tag), on_iteration=seen, replay=replay)
    assert st.iteration == [1, 2] and all(np.isfinite(st.loss)) and len(got) == 2
    return got, st


def test_loop_device_replay_alone_trains_what_the_default_loop_trains(tmp_path):
    (d1, d2), sd = _loop(tmp_path, "default")
    (r1, r2), sr = _loop(tmp_path, "device", device_replay=True)
    assert d1.tobytes() == r1.tobytes() and d2.tobytes() == r2.tobytes()
    assert sd.loss == sr.loss
    for gd, gr in zip(sd.games_played, sr.games_played):
        assert set(gd) == {"games_amnt", "positions_retrieved"}
        assert gr == dict(gd, window_records=gd["positions_retrieved"])


def test_loop_with_a_window_of_two_and_merging(tmp_path):
    seen = []
    with ReplayBuffer(capacity=180_000, window=2) as buf:
        def look(it):
            raw, _ = buf.fetch(merge=False)
            raw = raw.copy()
            out, mult = buf.fetch(merge=True)
            ro, rm = rr.merge(raw)
            assert out.tobytes() == ro.tobytes() and np.array_equal(mult, rm)
            seen.append((len(raw), len(out)))

        _, st = _loop(tmp_path, "window", replay=buf, on_iteration=look, replay_iterations=2, merge_duplicates=True)
    g1, g2 = st.games_played
    assert g1["window_records"] == g1["positions_retrieved"]
    assert g2["window_records"] == g1["positions_retrieved"] + g2["positions_retrieved"]
    for g, (n_raw, n_merged) in zip((g1, g2), seen):
        assert g["unique_records"] <= g["window_records"]
        assert (g["window_records"], g["unique_records"]) == (n_raw, n_merged)
