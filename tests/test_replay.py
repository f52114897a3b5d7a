"""CPU: the replay buffer's merge rule on the host and the pieces of the loop around it (include/onitama_az.h,
"replay buffer").

oaz_replay_merge_host against the numpy restatement (replay_ref): bytes, multiplicities and order; a group of
one is verbatim; merging is idempotent and does not depend on the members' order; train_epochs_device draws what
train_epochs draws and binds instead of loading; the LoopConfig defaults and the config's layout; and the host
rule, built alone with the address and undefined-behaviour sanitizers, in a program of its own. No GPU.
"""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import replay_ref as rr
from onitama_az import _abi
from onitama_az import replay
from onitama_az import trainer as trn

ROOT = Path(__file__).resolve().parents[1]


def _same(got, ref):
    (go, gm), (ro, rm) = got, ref
    assert len(go) == len(ro) and np.array_equal(gm, rm) and gm.dtype == np.uint32
    assert go.tobytes() == ro.tobytes()


def _check(samples):
    got = replay.merge_host(samples)
    _same(got, rr.merge(samples))
    return got


# ---- the rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single(n):
    out, mult = _check(rr.synthetic(np.arange(n), seed=1))
    assert len(out) == n and mult.tolist() == [1] * n


def test_thousand_distinct_records_come_back_verbatim():
    s = rr.synthetic(np.arange(1000), seed=2)
    out, mult = _check(s)
    assert out.tobytes() == s.tobytes() and np.all(mult == 1)


def test_thousand_copies_of_one_key():
    s = rr.synthetic(np.zeros(1000, dtype=np.int64), seed=3)
    assert set(np.unique(s["z"]).tolist()) == set(rr.Z_VALUES)
    out, mult = _check(s)
    assert mult.tolist() == [1000] and out["state"].tobytes() == s["state"][:1].tobytes()
    # the means, to float32's precision (the bytes are the restatement's, above)
    assert np.allclose(out["pi"][0], s["pi"].astype(np.float64).mean(0), rtol=0, atol=1e-7)
    assert abs(float(out["z"][0]) - s["z"].astype(np.float64).mean()) < 1e-7


def test_mix_of_forty_keys():
    mults = np.random.default_rng(4).integers(1, 301, 40)
    mults[:3] = (1, 300, 2)
    s = rr.synthetic(rr.mixed_ids(mults, seed=5), seed=6)
    out, mult = _check(s)
    assert len(out) == 40 and int(mult.sum()) == len(s) and sorted(mult.tolist()) == sorted(mults.tolist())


def test_keys_that_differ_in_one_field_stay_apart():
    base = rr.synthetic(np.zeros(1, dtype=np.int64), seed=7)[0]
    base["state"]["kings"] = (1 << 20, 1 << 9)
    variants = []
    for change in ("none", "to_move", "card", "pawn", "kings"):
        r = base.copy()
        if change == "to_move":
            r["state"]["to_move"] ^= 1
        elif change == "card":
            r["state"]["cards"][4] = 9
        elif change == "pawn":
            r["state"]["pawns"][1] ^= 1 << 31
        elif change == "kings":
            r["state"]["kings"] = (1 << 9, 1 << 20)  # the two kings exchanged
        variants.append(r)
    s = np.array(variants + variants, dtype=_abi.SAMPLE_DTYPE)  # every variant twice
    s["pi"][5:] = s["pi"][5:][:, ::-1]
    out, mult = _check(s)
    assert mult.tolist() == [2] * 5 and out["state"].tobytes() == s["state"][:5].tobytes()


def test_pad_is_not_part_of_the_key_and_the_representative_keeps_its_own():
    s = rr.synthetic(np.zeros(3, dtype=np.int64), seed=8)
    s["state"]["pad"] = [(7, 9), (1, 2), (3, 4)]
    out, mult = _check(s)
    assert mult.tolist() == [3] and out["state"]["pad"].tolist() == [[7, 9]]
    assert rr.key_bytes(s[0]) == rr.key_bytes(s[1]) and s["state"][0].tobytes() != s["state"][1].tobytes()


def test_a_group_of_one_is_verbatim_where_the_fixed_point_would_lose_bits():
    s = rr.synthetic(np.arange(4), seed=9)
    tiny = np.float32(2.0 ** -9) * np.float32(1 - 2.0 ** -24)  # 24 significant bits below 2^-9: not a multiple of 2^-32
    s["pi"][:, 3] = tiny
    s["pi"][:, 4] = np.float32(1e-30)
    s["z"][1] = np.float32(0.3)
    assert np.float32(np.rint(np.float64(tiny) * rr.TWO32) / rr.TWO32) != tiny  # F does lose bits here
    out, mult = _check(s)
    assert np.all(mult == 1) and out.tobytes() == s.tobytes()
    two = np.concatenate([s[:1], s[:1]])  # and in a group of two the entry goes through F
    out, _ = _check(two)
    assert out["pi"][0, 3] != tiny and out["pi"][0, 4] == 0


def test_merging_is_idempotent():
    s = rr.synthetic(rr.mixed_ids([5, 1, 40, 2, 1, 9], seed=10), seed=11)
    once = replay.merge_host(s)
    twice = replay.merge_host(once[0])
    assert twice[0].tobytes() == once[0].tobytes() and np.all(twice[1] == 1)


def test_the_order_of_a_groups_members_after_the_first_does_not_matter():
    ids = rr.mixed_ids([30, 7, 1, 12], seed=12)
    s = rr.synthetic(ids, seed=13)
    want = replay.merge_host(s)
    rng = np.random.default_rng(14)
    perm = np.arange(len(s))
    for k in range(4):  # shuffle each group's members after its first among the places they hold
        places = np.nonzero(ids == k)[0][1:]
        perm[places] = rng.permutation(places)
    assert np.any(perm != np.arange(len(s)))
    _same(replay.merge_host(s[perm]), want)


def test_argument_checks(lib):
    s = rr.synthetic(np.arange(2), seed=15)
    out = np.zeros(2, dtype=_abi.SAMPLE_DTYPE)
    n = C.c_size_t(5)
    assert lib.oaz_replay_merge_host(None, 2, _abi.ptr(out), None, C.byref(n)) == _abi.ERR_ARG
    assert lib.oaz_replay_merge_host(_abi.ptr(s), 2, None, None, None) == _abi.ERR_ARG
    assert lib.oaz_replay_merge_host(_abi.ptr(s), 2, _abi.ptr(out), None, None) == 0 and out.tobytes() == s.tobytes()
    assert lib.oaz_replay_merge_host(None, 0, None, None, C.byref(n)) == 0 and n.value == 0


# ---- the restated window (what tests/test_gpu_replay.py holds the device buffer to) -------------------------
def test_restated_window():
    segs = [np.zeros(k, dtype=_abi.SAMPLE_DTYPE) for k in (100, 0, 200, 50, 300)]
    assert [len(s) for s in rr.window(segs, 3, 10 ** 6)] == [200, 50, 300]
    assert [len(s) for s in rr.window(segs, 3, 400)] == [50, 300]
    assert [len(s) for s in rr.window(segs[:3], 3, 400)] == [100, 0, 200]
    assert [len(s) for s in rr.window(segs + [np.zeros(401, dtype=_abi.SAMPLE_DTYPE)], 3, 400)] == [50, 300]
    assert [len(s) for s in rr.window(segs, 1, 250)] == [50]  # the 300 were refused: more than the capacity
    assert [len(s) for s in rr.window(segs, 2, 320)] == [300]  # 50 + 300 are too many, one segment always stays


# ---- epoch drivers ------------------------------------------------------------------------------------------
class StubTrainer:
    """Records what the epoch drivers upload and how the data was attached."""

    def __init__(self):
        self.uploads, self.attached = [], []

    def load_samples(self, samples):
        self.attached.append(("load", len(samples)))

    def bind_device_samples(self, ptr, n):
        self.attached.append(("bind", ptr, n))

    def set_batches(self, idx, reflect=None):
        self.uploads.append((np.array(idx, dtype=np.int32), None if reflect is None else np.array(reflect)))
        self.k = len(idx)

    def train(self, first, count):
        assert (first, count) == (0, self.k)

    def losses(self):
        return 2.0 * self.k, 4.0 * self.k, self.k


@pytest.mark.parametrize("reflect", [0, 1, 2])
def test_train_epochs_device_draws_what_train_epochs_draws(reflect):
    n, batch, epochs, seed = 100, 16, 3, 11
    a, b = StubTrainer(), StubTrainer()
    ha = trn.train_epochs(a, np.zeros(n, dtype=_abi.SAMPLE_DTYPE), epochs=epochs, batch=batch, seed=seed, reflect=reflect)
    hb = trn.train_epochs_device(b, 0xABC000, n, epochs=epochs, batch=batch, seed=seed, reflect=reflect)
    assert a.attached == [("load", n)] and b.attached == [("bind", 0xABC000, n)]
    assert ha == hb and len(a.uploads) == len(b.uploads) == epochs
    for (ia, fa), (ib, fb) in zip(a.uploads, b.uploads):
        assert np.array_equal(ia, ib) and ia.shape == ((2 if reflect == 2 else 1) * n // batch, batch)
        assert (fa is None) == (fb is None) == (reflect == 0) and (fa is None or np.array_equal(fa, fb))
    # fewer records than a batch: no epoch, as train_epochs
    c = StubTrainer()
    assert trn.train_epochs_device(c, 0xABC000, batch - 1, epochs=2, batch=batch, seed=seed) == [] and not c.uploads


# ---- configuration ------------------------------------------------------------------------------------------
def test_loop_config_defaults_and_config_layout(lib):
    from onitama_az.train_loop import LoopConfig
    c = LoopConfig()
    assert (c.replay_iterations, c.merge_duplicates, c.device_replay, c.buffer_size) == (1, False, False, 180_000)
    cfg = _abi.oaz_replay_config()
    cfg.capacity, cfg.window, cfg.device, cfg.table_slots, cfg.pad = 1, 2, 3, 4, 5
    lib.oaz_replay_config_default(C.byref(cfg))
    assert (cfg.capacity, cfg.window, cfg.device, cfg.table_slots, cfg.pad) == (180_000, 1, 0, 0, 0)
    t = _abi.oaz_replay_config
    assert C.sizeof(t) == 24 and (t.capacity.offset, t.window.offset, t.device.offset, t.table_slots.offset,
                                  t.pad.offset) == (0, 8, 12, 16, 20)
    assert C.sizeof(_abi.oaz_replay_stats) == 56 and [f for f, _ in _abi.oaz_replay_stats._fields_] == [
        "segments", "records", "unique", "max_mult", "appended", "evicted", "probes"]
    assert lib.oaz_abi_version() == 5 and _abi.ERR_INTERNAL == -9
    # create checks its arguments before it looks for a device
    for bad in (dict(capacity=0), dict(capacity=1 << 31), dict(window=0)):
        with pytest.raises(_abi.OazError):
            replay.ReplayBuffer(**bad)


# ---- the host rule under the sanitizers -----------------------------------------------------------------------
def test_host_rule_alone_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/oaz_replay_host.cpp holds no HIP, so it builds with the host compiler alone: with
    tests/c/replay_merge_main.cpp (its own main, the mixed input) and -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "replay_merge_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests/c/replay_merge_main.cpp"),
                    str(ROOT / "onitama-alphazero_amd/csrc/oaz_replay_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "replay_merge_host OK" in run.stdout, run.stdout + run.stderr
