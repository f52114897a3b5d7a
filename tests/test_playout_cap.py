"""CPU: playout cap randomization (oaz_selfplay_set_playout_cap). The host restatement oaz_playout_cap_full against
the Python one over the oracle's Philox (tests/playout_cap_util.py), the share of full plies it gives, the argument
errors that need no device, the exports, the training loop's options, and the schedule of a capped self-play ply:
tests/c/playout_cap_schedule.cpp is tests/c/engine_schedule.cpp (unchanged, its main defined away) with recording
fakes of the two new launchers, linked with the real csrc/oaz_engine.cpp compiled host-only. Needs no GPU.

tests/golden/playout_cap_schedule_off.txt is what the engine of the commit before the cap enqueued for the two
scenarios without a cap, recorded from that commit's csrc with the same recorder (from the repository root):

    hipcc <FLAGS below> -DPLAYOUT_CAP_OFF_ONLY tests/c/playout_cap_schedule.cpp \\
        onitama-alphazero_amd/csrc/oaz_engine.cpp onitama-alphazero_amd/csrc/oaz_pack.cpp -o playout_cap_schedule
    ./playout_cap_schedule > tests/golden/playout_cap_schedule_off.txt
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import playout_cap_util as pcu
from onitama_az import _abi
from test_engine_schedule import CSRC, FLAGS, ROOT, _hipcc, _scenarios

GOLDEN_OFF = ROOT / "tests" / "golden" / "playout_cap_schedule_off.txt"
SHARES = (0, 1, 16384, 65535, 65536)
SIMS, FAST = 18, 5  # the recorder's scenarios


def _host_full(lib, seed, gid, ply, P):
    return lib.oaz_playout_cap_full(C.c_uint64(seed), C.c_uint64(gid), C.c_uint32(ply), C.c_uint32(P))


def test_p1_host_rule_equals_the_restatement(lib, orc):
    gids = list(range(8)) + [2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 63 + 11]
    seen = {P: set() for P in SHARES}
    for seed in (20260107, 2 ** 64 - 1):
        for gid in gids:
            for ply in range(256):
                for P in SHARES:
                    want = pcu.is_full(orc, seed, gid, ply, P)
                    assert _host_full(lib, seed, gid, ply, P) == int(want), (seed, gid, ply, P)
                    seen[P].add(want)
    assert seen[0] == {False} and seen[65536] == {True}  # none, all
    assert seen[16384] == {False, True} and True in seen[65535] and False in seen[1]
    # the ply and the game id enter the counter (both halves of the id)
    row = [_host_full(lib, 20260107, 3, ply, 16384) for ply in range(256)]
    assert row != [_host_full(lib, 20260107, 4, ply, 16384) for ply in range(256)]
    assert row != [_host_full(lib, 20260107, 3 + 2 ** 32, ply, 16384) for ply in range(256)]
    assert 0 < sum(row) < 256


def test_p1_share_of_full_plies(lib, orc):
    """Seed 20260107, game ids 0..4095, plies 0..15, P = 16384: the rule (computed from the oracle's generator) gives
    16 135 full plies of 65 536. Pinned: the +-4 sigma band around the expected 16 384 (sigma = sqrt(65 536 * 1/4 *
    3/4) = 110.9), 15 940..16 828, on the host function and on the restatement; counter-based, so it cannot flake."""
    seed, P = 20260107, 16384
    host = sum(_host_full(lib, seed, gid, ply, P) for gid in range(4096) for ply in range(16))
    rule = sum(pcu.is_full(orc, seed, gid, ply, P) for gid in range(4096) for ply in range(16))
    print("full plies of 65536: host", host, "restatement", rule)
    assert 15940 <= host <= 16828 and 15940 <= rule <= 16828
    assert host == rule


def test_p2_argument_errors_without_a_device(lib):
    assert _host_full(lib, 1, 2, 3, 65537) == _abi.ERR_ARG
    assert _host_full(lib, 1, 2, 3, 2 ** 32 - 1) == _abi.ERR_ARG
    assert _host_full(lib, 1, 2, 3, 65536) == 1 and _host_full(lib, 1, 2, 3, 0) == 0
    for fast, share in ((4, 16384), (0, 0), (-1, 16384), (4, -1), (4, 65537)):
        assert lib.oaz_selfplay_set_playout_cap(None, fast, share) == _abi.ERR_ARG
    assert lib.oaz_selfplay_playout_cap_stats(None, None) == _abi.ERR_ARG
    from onitama_az.engine import playout_cap_full
    assert playout_cap_full(1, 2, 3, 65536) is True and playout_cap_full(1, 2, 3, 0) is False
    with pytest.raises(_abi.OazError):
        playout_cap_full(1, 2, 3, 65537)


def test_p2_exports_and_layout(lib):
    header = (ROOT / "include" / "onitama_az.h").read_text()
    for name in ("oaz_playout_cap_full", "oaz_selfplay_set_playout_cap", "oaz_selfplay_playout_cap_stats"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header), name
    assert lib.oaz_abi_version() == _abi.ABI_VERSION == 5 and C.sizeof(_abi.oaz_config) == 120  # an engine setting


def test_p2_loop_config_reaches_the_engine(monkeypatch, tmp_path):
    """train_loop.train passes the two LoopConfig fields to the self-play engine, and nothing when the cap is off."""
    from onitama_az import train_loop

    d = train_loop.LoopConfig()
    assert (d.playout_cap_fast_sims, d.playout_cap_full) == (0, 16384)

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

    for cfg, want in ((train_loop.LoopConfig(iterations=1), None),
                      (train_loop.LoopConfig(iterations=1, playout_cap_fast_sims=100, playout_cap_full=8192), (100, 8192))):
        seen = {}

        def fake_engine(*a, **kw):
            seen.update(kw)
            raise Stop

        monkeypatch.setattr(train_loop, "Trainer", FakeTrainer)
        monkeypatch.setattr(train_loop, "Engine", fake_engine)
        with pytest.raises(Stop):
            train_loop.train(cfg, folder=str(tmp_path), initial_weights=np.zeros(4, np.float32))
        assert seen.get("playout_cap") == want and seen["sims"] == 400


# ---- the schedule of a capped ply ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schedule(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("playout_cap_schedule") / "playout_cap_schedule"
    srcs = [ROOT / "tests/c/playout_cap_schedule.cpp", CSRC / "oaz_engine.cpp", CSRC / "oaz_pack.cpp"]
    subprocess.run([hipcc, *FLAGS, *map(str, srcs), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert not [ln for ln in out if "LEAKED" in ln or "!dead" in ln]
    return _scenarios(out)


def _launches(lines):
    """[(number, kernel, stream, {key: value})] of a scenario's launch lines."""
    out = []
    for ln in lines:
        if ln.startswith("#"):
            w = ln.split()
            out.append((int(w[0][1:]), w[1], w[2], dict(x.split("=", 1) for x in w[3:])))
    return out


def _at(ptr, off):
    """The log's name of `off` bytes past a device pointer."""
    a, b = ptr.split("+")
    return f"{a}+{int(b) + off}"


def test_p3_a_cap_off_engine_enqueues_what_it_did(schedule):
    want = _scenarios(GOLDEN_OFF.read_text().splitlines())
    assert list(want) == ["off, 129 games, 1 part", "off, 2050 games, 2 parts", "end"]
    for title in list(want)[:2]:
        assert len(want[title]) > 80
        assert schedule[title] == want[title], title
        assert not [ln for ln in schedule[title] if "playout_cap" in ln or "selfplay_move_cap" in ln]


@pytest.mark.parametrize("games,parts", [(129, 1), (2050, 2)])
def test_p3_capped_ply_schedule(schedule, games, parts):
    title = f"cap {FAST} of {SIMS}, {games} games, {parts} part" + ("s" if parts > 1 else "")
    lines = schedule[title]
    assert "set_playout_cap rc=0" in lines and "selfplay_step rc=0" in lines
    # the cap's buffers come with the setter: the allocations of the cap-off engine of this size, then three more
    off = schedule[title.replace(f"cap {FAST} of {SIMS}", "off")]
    n_off = max(int(m) for ln in off for m in re.findall(r"\ba(\d+)\+", ln))
    L = _launches(lines)
    masks = [x for x in L if x[1] == "playout_cap_masks"]
    assert len(masks) == 1
    mk = masks[0][3]
    assert mk["slots"] == str(games) and mk["P"] == "16384"
    assert [mk[k].split("+")[0] for k in ("full", "nrec", "cnt")] == [f"a{n_off + i}" for i in (1, 2, 3)]
    active, fast, fullm = mk["active"], mk["fast"], mk["fullm"]
    assert (fast, fullm) == (_at(mk["full"], games), _at(mk["full"], 2 * games))
    assert active.split("+")[0] != fast.split("+")[0]
    # the mask kernel before the first select, the capped ply kernel last, and never the other ply kernels
    first_select = min(x[0] for x in L if x[1] == "select")
    assert masks[0][0] < first_select
    assert masks[0][0] < min(x[0] for x in L if x[1] == "root_noise")
    ply_launches = [x for x in L if x[1].startswith("selfplay_move")]
    assert [x[1] for x in ply_launches] == ["selfplay_move_cap"]
    assert ply_launches[0][0] == max(x[0] for x in L if x[1] != "stats_reduce")
    assert ply_launches[0][3]["full"] == mk["full"] and ply_launches[0][3]["nrec"] == mk["nrec"]
    assert not [x for x in L if x[1] in ("search_grp", "search_lat")]
    # per part (= per stream): the launches in order, and the mask each got
    each = (games + parts - 1) // parts
    streams = sorted({x[2] for x in L if x[1] == "select"})
    assert len(streams) == parts
    for h, st in enumerate(streams):
        g0 = h * each
        mine = [x for x in L if x[2] == st and x[1] in ("select", "backup_select", "expand_backup", "eval_compact",
                                                        "hash_eval")]
        names = [x[1] for x in mine]
        step = ["eval_compact", "hash_eval"]
        assert names == (["select"] + step + (["backup_select"] + step) * (FAST - 1) + ["expand_backup"] +
                         (["backup_select"] + step) * (SIMS - FAST) + ["expand_backup"])
        assert names.count("select") == 1 and names.count("backup_select") == (FAST - 1) + (SIMS - FAST)
        assert names.count("expand_backup") == 2 and names.count("eval_compact") == SIMS
        tree = [x for x in mine if x[1] in ("select", "backup_select", "expand_backup")]
        got = [x[3]["active"] for x in tree]
        assert got == ([_at(active, g0)] * FAST + [_at(fast, g0)] + [_at(fullm, g0)] * (SIMS - FAST) + [_at(fullm, g0)])
        assert all(x[3]["need"] == "1" and x[3]["slot"] == "1" for x in tree)  # leaf compaction on
    # the root noise: chunk 0 (simulations 0..15, phase one starts it) for every active game, chunk 1 (16, 17: the
    # chunk boundary lies inside phase two) for the full games only
    noise = [(x[3]["sim0"], x[3]["nsims"], x[3]["active"]) for x in L if x[1] == "root_noise"]
    assert noise == [("0", "16", active), ("16", "2", fullm)]


def test_p3_refusals_on_the_host(schedule):
    s = schedule["refusals"]
    assert "set_playout_cap(18) rc=0" in s  # fast_sims >= sims is the step's to refuse (sims may change)
    assert f"selfplay_step rc={_abi.ERR_STATE} error=selfplay_step: the playout cap's fast_sims=18 is not below sims=18" in s
    assert f"selfplay_step rc={_abi.ERR_STATE} error=selfplay_step: a playout cap does not run with a search-time budget" in s
    assert f"set_playout_cap(6) rc={_abi.ERR_STATE} error=set_playout_cap: the engine has a search-time budget" in s
    assert "set_playout_cap(0) rc=0" in s and "playout_cap_stats rc=0 full=0 fast=0" in s
    assert not [ln for ln in s if ln.startswith("#")]  # nothing was launched
