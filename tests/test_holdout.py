"""CPU: the held-out split (oaz_holdout_pick, oaz_holdout_mask_host; include/onitama_az.h, "held-out evaluation")
against the restatement in tests/train_eval_ref.py, the `subset` argument of the epoch drivers against a
recording stub trainer, and the added struct's size. No GPU."""
import ctypes as C

import numpy as np
import pytest

import train_eval_ref as ter
from conftest import random_positions
from onitama_az import _abi, holdout
from onitama_az import trainer as trn

SEED = 20260101


@pytest.fixture(scope="module")
def records(orc):
    """2,000 random-play positions as records with random pi and z (the rule looks at neither)."""
    rng = np.random.default_rng(3)
    s = np.zeros(2000, dtype=_abi.SAMPLE_DTYPE)
    s["state"] = random_positions(orc, 2000, seed=3)
    s["pi"] = rng.random((2000, 50)).astype(np.float32)
    s["z"] = rng.integers(-1, 2, 2000).astype(np.float32)
    s.setflags(write=False)
    return s


# ---- the rule ---------------------------------------------------------------------------------------------
def test_philox_restatement_known_answers():
    """Philox4x32-10 of the Random123 known-answer tests: the restatement is the published generator."""
    z = np.zeros(1, dtype=np.uint64)
    assert [int(w[0]) for w in ter.philox(z, z, z, z, z)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(w[0]) for w in ter.philox(np.full(1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), f, f, f, f)] == [
        0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("per", [1, 6554, 16384, 40000, 65535])
def test_mask_host_and_pick_equal_the_restatement(lib, records, per):
    want = ter.holdout_mask(records, SEED, per)
    got = holdout.mask(records, SEED, per)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    states = np.ascontiguousarray(records["state"])
    assert [int(holdout.pick(states[i], SEED, per)) for i in range(0, 2000, 7)] == want[::7].tolist()
    assert abs(int(want.sum()) - 2000 * per / 65536) < 5 * np.sqrt(2000 * 0.25) + 1  # the share is what was asked
    if 6554 <= per <= 40000:  # another seed, another split
        assert not np.array_equal(want, ter.holdout_mask(records, SEED + 1, per))


def test_none_and_all(lib, records):
    assert not holdout.mask(records, SEED, 0).any() and not ter.holdout_mask(records, SEED, 0).any()
    assert holdout.mask(records, SEED, 65536).all() and ter.holdout_mask(records, SEED, 65536).all()
    st = np.ascontiguousarray(records["state"][:1])
    assert holdout.pick(st[0], SEED, 0) is False and holdout.pick(st[0], SEED, 65536) is True


@pytest.mark.parametrize("n", [0, 1])
def test_mask_of_no_and_one_record(lib, records, n):
    got = holdout.mask(records[:n], SEED, 30000)
    assert got.shape == (n,) and np.array_equal(got, ter.holdout_mask(records[:n], SEED, 30000))
    assert lib.oaz_holdout_mask_host(None, 0, SEED, 30000, None) == 0  # n == 0: null pointers are fine


def test_argument_errors(lib, records):
    rec = np.ascontiguousarray(records[:4])
    out = np.zeros(4, dtype=np.uint8)
    st = np.ascontiguousarray(rec["state"])
    assert lib.oaz_holdout_pick(SEED, _abi.ptr(st), 65537) == _abi.ERR_ARG
    assert lib.oaz_holdout_pick(SEED, None, 100) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask_host(_abi.ptr(rec), 4, SEED, 65537, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask_host(None, 4, SEED, 100, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask_host(_abi.ptr(rec), 4, SEED, 100, None) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask_host(_abi.ptr(rec), 0, SEED, 65537, _abi.ptr(out)) == _abi.ERR_ARG
    # the device entry's checks are made before a device is touched
    assert lib.oaz_holdout_mask(None, 4, SEED, 100, 0, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask(_abi.ptr(rec), 4, SEED, 65537, 0, _abi.ptr(out)) == _abi.ERR_ARG
    assert lib.oaz_holdout_mask(None, 0, SEED, 100, 0, None) == 0
    with pytest.raises(_abi.OazError):
        holdout.mask(rec, SEED, 70000)


def test_equal_positions_fall_on_the_same_side_whatever_pi_z_and_pad(lib, records):
    a = np.ascontiguousarray(records[:500]).copy()
    b = a.copy()
    rng = np.random.default_rng(9)
    b["pi"] = rng.random((500, 50)).astype(np.float32)
    b["z"] = -a["z"]
    b["state"]["pad"] = rng.integers(1, 256, (500, 2))  # the pad bytes are no part of the key
    for per in (6554, 32768):
        ma, mb = holdout.mask(a, SEED, per), holdout.mask(b, SEED, per)
        assert np.array_equal(ma, mb) and np.array_equal(mb, ter.holdout_mask(b, SEED, per))
    both = np.concatenate([a, b])[rng.permutation(1000)]  # a window holding every position twice
    m = holdout.mask(both, SEED, 16384)
    side = {}
    for rec, f in zip(both, m):
        assert side.setdefault(rec["state"].tobytes()[:22], int(f)) == int(f)


def test_split():
    m = np.array([0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    tr_ids, ho_ids = holdout.split(m)
    assert tr_ids.dtype == ho_ids.dtype == np.int32
    assert tr_ids.tolist() == [0, 3, 4, 6] and ho_ids.tolist() == [1, 2, 5]
    e_tr, e_ho = holdout.split(np.zeros(0, dtype=np.uint8))
    assert len(e_tr) == len(e_ho) == 0 and e_tr.dtype == np.int32


# ---- sizes ------------------------------------------------------------------------------------------------
def test_struct_size_and_abi_version(lib):
    assert C.sizeof(_abi.oaz_eval_stats) == 64 and _abi.oaz_eval_stats.value_sq.offset == 32
    assert lib.oaz_abi_version() == 5 == _abi.ABI_VERSION
    for name in ("oaz_holdout_pick", "oaz_holdout_mask_host", "oaz_holdout_mask", "oaz_trainer_evaluate",
                 "oaz_trainer_predict"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_eval_stats_properties():
    e = trn.EvalStats(n=4, decided=2, top1=3, sign=1, value_sq_sum=2.0, policy_ce_sum=10.0, target_entropy_sum=4.0)
    assert (e.value_mse, e.policy_ce, e.policy_kl, e.top1_rate, e.sign_rate) == (0.5, 2.5, 1.5, 0.75, 0.5)
    assert e.policy_loss == 10.0 / (25 * 4)
    z = trn.EvalStats()
    assert (z.value_mse, z.policy_kl, z.sign_rate, z.policy_loss) == (0.0, 0.0, 0.0, 0.0)
    assert set(e.summary()) >= {"n", "value_mse", "policy_ce", "policy_kl", "policy_loss", "top1_rate", "sign_rate"}


# ---- the epoch drivers' subset ------------------------------------------------------------------------------
class StubTrainer:
    """Records what the epoch drivers upload."""

    def __init__(self):
        self.uploads = []

    def load_samples(self, samples):
        self.n = len(samples)

    def bind_device_samples(self, ptr, n):
        self.n = n

    def set_batches(self, idx, reflect=None):
        self.uploads.append((np.array(idx, dtype=np.int32), None if reflect is None else np.array(reflect)))
        self.k = len(idx)

    def train(self, first, count):
        assert (first, count) == (0, self.k)

    def losses(self):
        return 2.0 * self.k, 4.0 * self.k, self.k


def _uploads(reflect, subset, n=100, batch=16, epochs=3, seed=11, device=False):
    tr = StubTrainer()
    kw = {} if subset is None else {"subset": subset}
    if device:
        hist = trn.train_epochs_device(tr, 0x1000, n, epochs=epochs, batch=batch, seed=seed, reflect=reflect, **kw)
    else:
        hist = trn.train_epochs(tr, np.zeros(n, dtype=_abi.SAMPLE_DTYPE), epochs=epochs, batch=batch, seed=seed,
                                reflect=reflect, **kw)
    assert len(hist) == len(tr.uploads)
    return tr.uploads


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("reflect", [0, 1, 2])
def test_subset_none_draws_the_streams_of_the_seed(reflect, device):
    """Without a subset the index and flag streams are those the drivers drew before they had the argument:
    choose_batches / choose_reflect / choose_batches_doubled on default_rng(seed) and the flags' own generator."""
    got = _uploads(reflect, None, device=device)
    rng, frng = np.random.default_rng(11), np.random.default_rng([trn.REFLECT_TAG, 11])
    assert len(got) == 3
    for idx, flags in got:
        if reflect == 2:
            virt = trn.choose_batches(rng, 200, 16, 200 // 16)
            assert np.array_equal(idx, virt % 100) and np.array_equal(flags, (virt >= 100).astype(np.uint8))
        else:
            assert np.array_equal(idx, trn.choose_batches(rng, 100, 16, 100 // 16))
            assert (flags is None) if reflect == 0 else np.array_equal(flags, trn.choose_reflect(frng, idx.shape))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("reflect", [0, 1, 2])
def test_subset_batches_hold_its_members_only(reflect, device):
    subset = np.sort(np.random.default_rng(4).choice(100, 53, replace=False)).astype(np.int32)
    got = _uploads(reflect, subset, device=device)
    rng = np.random.default_rng(11)
    assert len(got) == 3
    for idx, flags in got:
        m = 2 * 53 if reflect == 2 else 53
        assert idx.shape == (m // 16, 16) and idx.dtype == np.int32  # an epoch is len(subset) // batch batches
        assert np.isin(idx, subset).all()
        pos = trn.choose_batches(rng, m, 16, m // 16)  # a batch is subset[choose_batches(rng, len(subset), ...)]
        assert np.array_equal(idx, subset[pos % 53])
        if reflect == 2:
            assert np.array_equal(flags, (pos >= 53).astype(np.uint8))
        for row_i, row_f in zip(idx, flags if flags is not None else np.zeros_like(idx)):
            assert len({(int(i), int(f)) for i, f in zip(row_i, row_f)}) == 16  # still without replacement


def test_subset_smaller_than_a_batch_trains_nothing_and_bad_members_are_refused():
    assert _uploads(0, np.arange(10, dtype=np.int32)) == []
    with pytest.raises(ValueError):
        _uploads(0, np.array([0, 100], dtype=np.int32))
    with pytest.raises(ValueError):
        _uploads(0, np.array([-1, 5], dtype=np.int32))


def test_subset_data_parallel_slices_line_up():
    subset = np.arange(3, 100, 2, dtype=np.int32)
    for reflect in (0, 1, 2):
        def draw(rank, world):
            rng, frng = np.random.default_rng(5), np.random.default_rng([trn.REFLECT_TAG, 5])
            return [trn.epoch_batches(rng, frng, len(subset), 32, reflect, rank, world, subset) for _ in range(2)]

        whole, parts = draw(0, 1), [draw(r, 2) for r in range(2)]
        for e, (idx, flags) in enumerate(whole):
            assert np.isin(idx, subset).all()
            assert np.array_equal(np.hstack([parts[r][e][0] for r in range(2)]), idx)
            if flags is not None:
                assert np.array_equal(np.hstack([parts[r][e][1] for r in range(2)]), flags)


def test_loop_config_defaults_are_off():
    from onitama_az.train_loop import LoopConfig, Stats
    c = LoopConfig()
    assert c.holdout_per_65536 == 0 and c.evaluate is False and Stats().evaluation == []
