"""CPU: the self-play temperature rule (oaz_config.temperature_plies). The host restatement oaz_temperature_pick
against the Python one over the oracle's Philox (tests/temperature_util.py), the distribution of the draws, and
the layout of the new config byte. Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import temperature_util as tu
from onitama_az import _abi

SEED = 20260101


def _host_pick(lib, seed, gid, ply, visits):
    v = np.ascontiguousarray(visits, dtype=np.uint32)
    return lib.oaz_temperature_pick(C.c_uint64(seed), C.c_uint64(gid), C.c_uint32(ply), _abi.ptr(v) if len(v) else None,
                                    len(v))


VECTORS = {
    "K=1": [7],
    "K=40, visits in 33..39 only": [0] * 33 + [5, 1, 9, 2, 30, 1, 152],
    "K=40, all visited": list(range(1, 41)),
    "leading and trailing zeros": [0, 0, 0, 4, 0, 11, 1, 0, 0],
    "one visit": [0, 0, 1, 0],
    "S=0": [0, 0, 0, 0, 0],
    "K=0": [],
    "S near 2^31": [2 ** 30, 5, 2 ** 30 - 3, 0, 1],
    "S near 2^32": [2 ** 31, 2 ** 31 - 1],
}


@pytest.mark.parametrize("name", list(VECTORS))
def test_t1_host_pick_equals_the_restatement(lib, orc, name):
    visits = VECTORS[name]
    gids = list(range(24)) + [2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 63 + 11]
    plies = [0, 1, 2, 7, 29, 151, 254, 255, 65536]
    seen = set()
    for seed in (SEED, 0, 2 ** 64 - 1):
        for gid in gids:
            for ply in plies:
                want = tu.pick(orc, seed, gid, ply, visits)
                got = _host_pick(lib, seed, gid, ply, visits)
                assert got == (-1 if want is None else want), (seed, gid, ply)
                assert want is None or visits[want] > 0
                seen.add(want)
    if sum(visits) == 0:
        assert seen == {None}
    else:
        assert None not in seen
        if name == "K=40, visits in 33..39 only":
            assert min(seen) >= 33 and 39 in seen and len(seen) >= 4


def test_t1_null_visits_draw_nothing(lib):
    assert lib.oaz_temperature_pick(C.c_uint64(1), C.c_uint64(2), C.c_uint32(0), None, 3) == -1
    v = np.array([3, 4], dtype=np.uint32)
    assert lib.oaz_temperature_pick(C.c_uint64(1), C.c_uint64(2), C.c_uint32(0), _abi.ptr(v), -1) == -1


def test_t2_distribution(lib):
    """100 000 game ids at one ply and seed. The draws are counter-based, hence the same on every run: this seed
    gives the counts [0, 225, 737, 0, 2971, 96067] (expected 250, 750, 3 000, 96 000), the largest deviation 1.58
    sigma of the binomial's, so the 5 sigma bound holds and the test cannot flake."""
    visits = np.array([0, 1, 3, 0, 12, 384], dtype=np.uint32)
    n, ply, S = 100_000, 3, int(visits.sum())
    draws = np.array([_host_pick(lib, SEED, gid, ply, visits) for gid in range(n)])
    counts = np.bincount(draws, minlength=len(visits))
    assert counts.sum() == n and draws.min() >= 0
    worst = 0.0
    for j, v in enumerate(visits):
        if v == 0:
            assert counts[j] == 0, j  # a child without visits is never played
            continue
        p = int(v) / S
        sigma = (n * p * (1 - p)) ** 0.5
        dev = abs(counts[j] - n * p) / sigma
        worst = max(worst, dev)
        assert dev <= 5.0, (j, counts[j], n * p, sigma)
    print("counts", counts.tolist(), "largest deviation %.2f sigma" % worst)
    # deterministic
    again = np.array([_host_pick(lib, SEED, gid, ply, visits) for gid in range(2000)])
    assert np.array_equal(again, draws[:2000])
    # the ply enters the counter: the same game draws another child at the next ply, for some games
    nxt = np.array([_host_pick(lib, SEED, gid, ply + 1, visits) for gid in range(2000)])
    assert 0 < (nxt != draws[:2000]).sum() < 2000
    # and so does the seed
    other = np.array([_host_pick(lib, SEED + 1, gid, ply, visits) for gid in range(2000)])
    assert (other != draws[:2000]).any()


def test_t3_layout_and_defaults(lib):
    assert C.sizeof(_abi.oaz_config) == 120 and _abi.oaz_config.temperature_plies.offset == 69
    assert _abi.oaz_config.pad0.offset == 70 and _abi.oaz_config.pad0.size == 2 and _abi.oaz_config.seed.offset == 72
    assert lib.oaz_abi_version() == _abi.ABI_VERSION == 5
    cfg = _abi.default_config()
    assert cfg.temperature_plies == 0 and bytes(cfg)[69:72] == b"\0\0\0"
    cfg.temperature_plies = 255
    assert bytes(cfg)[69] == 255 and bytes(cfg)[70:72] == b"\0\0"
    for name in ("oaz_temperature_pick", "oaz_search_sample_moves", "oaz_selfplay_temperature_stats"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_t3_loop_config_reaches_the_engine(monkeypatch, tmp_path):
    """train_loop.train passes LoopConfig.temperature_plies to the self-play engine's keyword arguments."""
    from onitama_az import train_loop

    assert train_loop.LoopConfig().temperature_plies == 0
    seen = {}

    class Stop(Exception):
        pass

    class FakeTrainer:
        def __init__(self, **kw):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def set_weights(self, w):
            pass

    def fake_engine(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(train_loop, "Trainer", FakeTrainer)
    monkeypatch.setattr(train_loop, "Engine", fake_engine)
    cfg = train_loop.LoopConfig(temperature_plies=8, iterations=1)
    with pytest.raises(Stop):
        train_loop.train(cfg, folder=str(tmp_path), initial_weights=np.zeros(4, np.float32))
    assert seen["temperature_plies"] == 8 and seen["reuse_visits"] == 0
