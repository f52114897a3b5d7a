"""CPU: the float64 reference of the network forward (tests/nn_ref.py) and the proof that the GPU
comparisons of tests/test_gpu_nn_ref.py can see a wrong kernel. No GPU.

  - `exact` mode against every torch fp32 golden set;
  - the conditions on the exact-integer nets of comparison (a) and on the value nets of (d);
  - the bars of (a) and (b), derived from the reference's own float32 runs;
  - planted defects: each GPU comparison's input set and nets move the reference by at least 10x that
    comparison's bar for every defect marked Y below.

Comparisons (columns): a0-a6 the exact-integer towers at depth 0, 1, 2, 3, 5, 6 (all precisions, bar
BAR_A); b0, b1 OAZ_BF16 at depth 0 / 1 on ordinary random nets (bar BAR_B, bf16-mode reference);
c3, c5, c6 OAZ_BF16 on trained3, trained5, random6 (bar 4x the reference's float64-versus-float32
accumulation distance); dF, dX, dH the value-head nets on OAZ_FP32 (1e-4), OAZ_FP32_SPLIT (1e-4),
OAZ_FP32_SPLIT16 (1e-5) against the exact reference; dB the same on OAZ_BF16 by (c)'s rule.
Y: seen (moves the reference >= 10x the bar; in b on more positions than may be excluded);
n: not seen by this comparison; -: the defect does not exist there (no second block, or no rounding
in an exact tower). In the c and dB columns, whose bar comes from a float32 run that differs between
BLAS builds, Y is claimed only above 20x.

DEFECT TABLE
defect                a0 a1 a2 a3 a5 a6 b0 b1 c3 c5 c6 dF dX dH dB
drop_tap              Y  Y  Y  Y  Y  Y  Y  Y  n  n  n  Y  Y  Y  n
swap_cin              Y  Y  Y  Y  Y  Y  Y  Y  n  n  n  Y  Y  Y  n
swap_cout             Y  Y  Y  Y  Y  Y  Y  Y  n  n  n  Y  Y  Y  n
block_weights         -  -  Y  Y  Y  Y  -  -  Y  Y  Y  Y  Y  Y  Y
skip_quantised        -  -  -  -  -  -  -  Y  n  n  n  -  -  -  n
truncate              -  -  -  -  -  -  Y  Y  n  n  n  -  -  -  n
unquantised_w         -  -  -  -  -  -  -  Y  n  n  n  -  -  -  n
unquantised_head_w    -  -  -  -  -  -  Y  Y  n  n  n  -  -  -  n
drop_value_feature    Y  Y  Y  Y  Y  n  Y  Y  n  n  n  Y  Y  Y  n
swap_policy_features  Y  Y  Y  Y  Y  Y  Y  Y  n  Y  n  Y  Y  Y  n
wrong_player_cards    Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
END TABLE
(a6 / drop_value_feature: value feature 7 is zero on every position of the depth-6 integer nets.)
"""
import numpy as np
import pytest

import nn_ref
import nn_ref_cases as cs
from onitama_az import _abi
from onitama_az.weights import named_from_blob

# exact mode against the torch fp32 goldens: measured 9.09e-7 (trained3), 1.71e-8 (random3), 1.04e-8
# (random6); the goldens are fp32, so their own rounding is the floor. Bar: 4x the largest.
GOLDEN_BAR = 4 * 9.1e-7


def _table():
    rows = __doc__.split("DEFECT TABLE\n")[1].split("END TABLE")[0].strip().splitlines()
    cols = rows[0].split()[1:]
    return cols, {r.split()[0]: dict(zip(cols, r.split()[1:])) for r in rows[1:]}


COLS, TABLE = _table()


def test_encoder_restatement_equals_oracle():
    assert np.array_equal(nn_ref.encode(cs.positions()), cs.planes())
    st = cs.positions()
    assert len(st) == 314 and len(st) % 16 != 0 and set(st["to_move"]) == {0, 1}
    # every card in both of the mover's slots, for both colours; one-hot boards on every square of every bitboard
    mover = {(int(s["to_move"]), k, int(s["cards"][2 * s["to_move"] + k])) for s in st[250:] for k in (0, 1)}
    assert {(c, k, card) for c in (0, 1) for k in (0, 1) for card in range(16)} <= mover
    assert (cs.planes()[150:250, :4].reshape(100, -1).sum(1) == 1).all()
    assert (cs.planes()[150:250, :4].reshape(4, 25, 4, 25).sum(1) > 0).sum() == 100


@pytest.mark.parametrize("name,blocks", [("trained3", 3), ("random3", 3), ("random6", 6)])
def test_exact_mode_matches_torch_goldens(nn_golden, trained3, name, blocks):
    from onitama_az.weights import random_weights
    w = trained3 if name == "trained3" else random_weights(0 if name == "random3" else 1, blocks)
    st = nn_golden["states"]
    r = nn_ref.forward(w, blocks, nn_ref.encode(st))
    d = nn_ref.distance(r, (nn_golden[f"policy_{name}"], nn_golden[f"value_{name}"]))
    print(f"exact reference vs torch fp32 golden {name}: {d:.3e}")
    assert d < GOLDEN_BAR


def test_bf16_rounding_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e-5, 0.0], dtype=np.float32)
    assert np.array_equal(nn_ref.bf16_rne(x)[:4], np.float32([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]))  # ties to even
    assert np.array_equal(nn_ref.bf16_trunc(x)[:4], np.float32([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0]))
    assert (nn_ref.bf16_rne(x).view(np.uint32) & 0xFFFF == 0).all()
    v = np.array([1.0 + 2.0 ** -8, (1.0 + 2.0 ** -8) * (1 + 2.0 ** -19), (1.0 + 2.0 ** -8) * (1 + 2.0 ** -17), 1.0, 0.0, -1.0])
    assert nn_ref.near_bf16_boundary(v).tolist() == [True, True, False, False, False, False]


# ---- (a) the exact-integer nets --------------------------------------------------------------------
@pytest.mark.parametrize("depth", cs.DEPTHS_A)
def test_integer_nets_conditions(depth):
    """Every condition of comparison (a), on the reference alone."""
    first = np.zeros((9, 21), dtype=bool)
    cin, cout = np.zeros((9, 64), dtype=bool), np.zeros((9, 64), dtype=bool)
    worst = 0.0
    assert 3 <= len(cs.integer_nets(depth)) <= 4
    for w, (r, acts) in zip(cs.integer_nets(depth), cs.integer_runs(depth)):
        named = named_from_blob(w, depth)
        convs = [("conv_init_1", "bn1")] + [(f"resnet_{i}|resnet_small_block{j}|small_block_conv",
                                             f"resnet_{i}|resnet_small_block{j}|small_block_bn")
                                            for i in range(depth) for j in (1, 2)]
        for k, (c, bn) in enumerate(convs):
            fw, fb = nn_ref.fold(named, c, bn)
            assert np.array_equal(fw, np.round(fw)) and np.array_equal(fb, np.round(fb))  # folded: exact integers
            nz = (fw != 0).reshape(64, -1, 9)
            if k == 0:
                first |= nz.any(0).T
            else:
                cin |= nz.any(0).T
                cout |= nz.any(1).T
        for c, bn in (("vh_conv", "vh_bn"), ("policy_conv", "policy_bn")):  # head convs: multiples of 1/8, bf16-exact
            fw, fb = nn_ref.fold(named, c, bn)
            assert np.array_equal(fw * 8, np.round(fw * 8)) and np.array_equal(fb * 8, np.round(fb * 8))
        for a in acts:
            assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() <= 256
        assert (acts[-1] > 0).mean() >= 0.10
        rb = nn_ref.forward(w, depth, cs.planes(), mode="bf16")
        assert np.array_equal(rb[0], r[0]) and np.array_equal(rb[1], r[1])  # bf16 mode bit-equal to exact
        p, v = r
        assert v.max() - v.min() >= 0.5 and np.abs(v).max() < 0.95 and p.max() < 0.9
        assert len(np.unique(p.reshape(len(v), 50), axis=0)) >= 0.9 * len(v)
        d = nn_ref.distance(nn_ref.forward(w, depth, cs.planes(), head_acc=np.float32, tower=acts[-1]), r)
        worst = max(worst, d)
    assert first.all()  # every (tap, plane) of the first layer carries a weight in some net
    if depth:
        assert cin.all() and cout.all()  # every (tap, input channel) and (tap, output channel) pair
    print(f"(a) depth {depth}: float64 vs float32 head MLPs {worst:.3e}; A_DIST {cs.A_DIST:.3e}")
    assert worst <= cs.A_DIST and cs.BAR_A == 8 * cs.A_DIST and cs.BAR_A <= 1e-5


# ---- (b) the shallow bf16 nets ---------------------------------------------------------------------
@pytest.mark.parametrize("depth", cs.DEPTHS_B)
def test_shallow_bf16_bar_and_exclusion_cap(depth):
    """BAR_B from the reference's float32-accumulation run, and that run itself under the GPU test's
    rule: the positions it puts beyond the bar are all near a bf16 rounding boundary and within the cap."""
    for w in cs.shallow_nets(depth):
        r64, r32, near, same = cs.bf16_pair(w, depth)
        pp = nn_ref.per_position(r32, r64)
        print(f"(b) depth {depth}: same roundings {int(same.sum())}/{len(same)}, distance there {pp[same].max():.3e}, "
              f"overall {pp.max():.3e}; beyond BAR_B {int((pp > cs.BAR_B).sum())}")
        assert same.sum() >= len(same) // 2
        assert pp[same].max() <= cs.B_DIST
        over = pp > cs.BAR_B
        assert not (over & ~near).any() and over.sum() <= cs.EXCLUDE_CAP * len(over)
    assert cs.BAR_B == max(cs.BAR_A, 8 * cs.B_DIST)


# ---- (d) the value nets ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", sorted(cs.VALUE_SEEDS))
def test_value_nets_span(precision):
    mode = "bf16" if precision == _abi.BF16 else "exact"
    p, v = nn_ref.forward(cs.value_net(precision), 3, cs.planes(), mode=mode)
    assert v.max() - v.min() >= 0.5 and np.abs(v).max() < 0.95 and p.max() < 0.9
    # its own fp32 summation noise stays well inside the tightest fp32-level bar (1e-5)
    if mode == "exact":
        assert nn_ref.distance(nn_ref.forward(cs.value_net(precision), 3, cs.planes(), acc=np.float32), (p, v)) < 2.5e-6


# ---- planted defects -------------------------------------------------------------------------------
def _comparison(col):
    """(nets, blocks, mode, bar, positions that must move) of one GPU comparison."""
    if col[0] == "a":
        d = int(col[1:])
        return cs.integer_nets(d), d, "exact", cs.BAR_A, 1
    if col[0] == "b":
        d = int(col[1:])
        return cs.shallow_nets(d), d, "bf16", cs.BAR_B, int(cs.EXCLUDE_CAP * len(cs.planes())) + 1
    if col[0] == "c":
        name = {"3": "trained3", "5": "trained5", "6": "random6"}[col[1:]]
        w = cs.deep_net(name)
        r64, r32, _, _ = cs.bf16_pair(w, cs.DEEP[name])
        return (w,), cs.DEEP[name], "bf16", 2 * 4 * nn_ref.distance(r32, r64), 1  # Y only above 20x
    prec = {"F": _abi.FP32, "X": _abi.FP32_SPLIT, "H": _abi.FP32_SPLIT16, "B": _abi.BF16}[col[1]]
    w = cs.value_net(prec)
    if prec == _abi.BF16:
        r64, r32, _, _ = cs.bf16_pair(w, 3)
        return (w,), 3, "bf16", 2 * 4 * nn_ref.distance(r32, r64), 1
    return (w,), 3, "exact", cs.FP32_BARS[prec], 1


@pytest.mark.parametrize("col", COLS)
def test_planted_defects_move_the_reference(col):
    nets, blocks, mode, bar, need = _comparison(col)
    exist = {d[0]: d for d in cs.defects(blocks) if mode == "bf16" or d[0] not in cs.ROUNDING_DEFECTS}
    bases = dict(enumerate(cs.integer_refs(blocks))) if col[0] == "a" else {}
    for name in nn_ref.DEFECTS:
        mark = TABLE[name][col]
        assert (mark == "-") == (name not in exist), (name, col)
        if mark != "Y":
            continue
        moved = np.zeros(len(cs.planes()))
        for k, w in enumerate(nets):
            if k not in bases:
                bases[k] = nn_ref.forward(w, blocks, cs.planes(), mode=mode)
            moved = np.maximum(moved, cs.moved_by(exist[name], w, blocks, mode, bases[k]))
            if (moved >= 10 * bar).sum() >= need:  # seen on this net: the others need not run
                break
        print(f"{col} {name}: moves the reference by {moved.max() / bar:.0f}x the bar, "
              f"{int((moved >= 10 * bar).sum())} positions >= 10x")
        assert (moved >= 10 * bar).sum() >= need, (name, col, moved.max() / bar)


def test_every_defect_is_seen_somewhere():
    assert set(TABLE) == set(nn_ref.DEFECTS)
    for name, row in TABLE.items():
        assert "Y" in row.values(), name
