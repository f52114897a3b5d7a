"""GPU: every NN kernel through Engine.nn_forward against the float64 reference (tests/nn_ref.py), on
nets and inputs at which the reference proves a wrong kernel would show (tests/test_nn_ref.py: the
defect x comparison table and the conditions on the nets).

  (a) exact-integer towers, all four precisions, depths 0, 1, 2, 3, 5, 6: every tower activation is a
      small integer, so every kernel must produce the same exact tower and only the fp32 head MLPs
      differ from float64; bar BAR_A; batches of 1, 15, 16, 17 and the whole set (314: a tail tile),
      for OAZ_FP32_SPLIT16 also 1,029, so that both k_nn_h3s and k_nn_h3 are compared;
  (b) OAZ_BF16 at depth 0 and 1 on ordinary random nets against the bf16-mode reference, bar BAR_B;
      a position may lie beyond the bar only where the reference itself shows a pre-rounding
      activation near a bf16 rounding boundary, and at most 2 % of the positions may;
  (c) OAZ_BF16 on trained3, trained5 and a random 6-block net: bar 4x the reference's own
      float64-versus-float32-accumulation distance, computed here from its two runs;
  (d) a 3-block net per precision whose value covers most of (-1, 1): the fp32-level kernels at
      1e-4 / 1e-4 / 1e-5 against the exact reference, OAZ_BF16 by (c)'s rule.
Each test prints the distance it measured before it asserts. Measured on an MI355X when written:
  (a) bar 3.68e-6: OAZ_FP32 and OAZ_FP32_SPLIT 2.1e-7 to 4.7e-7 per depth, OAZ_BF16 and
      OAZ_FP32_SPLIT16 2.3e-7 to 4.8e-7 (k_nn_h3s and k_nn_h3 alike), no fallback tile;
  (b) bar 3.68e-6: within it 4.2e-8 / 8.6e-8 (depth 0), 3.5e-6 / 3.3e-6 (depth 1); beyond it 1, 1, 1 and
      2 of 314 positions (6.3e-6 to 1.8e-5), all near a bf16 boundary by the reference;
  (c) trained3 3.5e-3 (bar 1.49e-2), trained5 4.4e-3 (2.21e-2), random6 3.2e-4 (8.4e-4);
  (d) OAZ_FP32 1.0e-6, OAZ_FP32_SPLIT 1.1e-6, OAZ_FP32_SPLIT16 5.2e-7, OAZ_BF16 3.9e-3 (bar 1.55e-2).
"""
import numpy as np
import pytest

import nn_ref
import nn_ref_cases as cs
from onitama_az import _abi
from onitama_az.engine import Engine

pytestmark = pytest.mark.gpu

NAMES = {_abi.FP32: "FP32", _abi.BF16: "BF16", _abi.FP32_SPLIT: "FP32_SPLIT", _abi.FP32_SPLIT16: "FP32_SPLIT16"}
BIG = 1024 + 5  # above one round of workgroups on any device: the tiled kernel, with a tail tile


def test_gpu_encoder_equals_reference_planes():
    from onitama_az.game import encode_batch
    assert np.array_equal(encode_batch(np.array(cs.positions())), cs.planes())


@pytest.mark.parametrize("depth", cs.DEPTHS_A)
@pytest.mark.parametrize("precision", sorted(NAMES))
def test_integer_towers_exact_on_every_kernel(precision, depth):
    st = np.array(cs.positions())
    n = len(st)
    big = np.ascontiguousarray(np.concatenate([st] * 4)[:BIG])
    worst = 0.0
    with Engine(games=BIG if precision == _abi.FP32_SPLIT16 else n, sims=1, blocks=depth, evaluator=_abi.EVAL_NN,
                precision=precision) as e:
        for w, ref in zip(cs.integer_nets(depth), cs.integer_refs(depth)):
            e.load_weights(w)
            for B in (1, 15, 16, 17, n):
                got = e.nn_forward(np.ascontiguousarray(st[:B]))
                worst = max(worst, nn_ref.distance(got, (ref[0][:B], ref[1][:B])))
            if precision == _abi.FP32_SPLIT16:
                idx = np.arange(BIG) % n
                worst = max(worst, nn_ref.distance(e.nn_forward(big), (ref[0][idx], ref[1][idx])))
        assert e.nn_fallbacks() == 0
    print(f"NNREF a depth {depth} {NAMES[precision]}: distance {worst:.3e} bar {cs.BAR_A:.3e}")
    assert worst <= cs.BAR_A


@pytest.mark.parametrize("depth", cs.DEPTHS_B)
def test_bf16_rounding_points_at_shallow_depth(depth):
    st = np.array(cs.positions())
    n = len(st)
    with Engine(games=n, sims=1, blocks=depth, evaluator=_abi.EVAL_NN, precision=_abi.BF16) as e:
        for k, w in enumerate(cs.shallow_nets(depth)):
            info = {}
            ref = nn_ref.forward(w, depth, cs.planes(), mode="bf16", info=info)
            e.load_weights(w)
            pp = nn_ref.per_position(e.nn_forward(st), ref)
            over = pp > cs.BAR_B
            print(f"NNREF b depth {depth} net {k}: distance within the bar {pp[~over].max():.3e} bar {cs.BAR_B:.3e}; "
                  f"beyond it {int(over.sum())} of {n} positions (largest {pp.max():.3e}), "
                  f"{int((over & ~info['near']).sum())} of them not near a bf16 boundary")
            assert not (over & ~info["near"]).any()
            assert over.sum() <= cs.EXCLUDE_CAP * n
            for B in (1, 17):  # the small-batch launch: the same arithmetic
                pb = nn_ref.per_position(e.nn_forward(np.ascontiguousarray(st[:B])), (ref[0][:B], ref[1][:B]))
                assert (pb <= cs.BAR_B)[~over[:B]].all()
        assert e.nn_fallbacks() == 0


def _bf16_by_noise_bar(tag, w, blocks):
    """(c)'s rule: OAZ_BF16 within 4x the reference's float64-vs-float32-accumulation distance."""
    st = np.array(cs.positions())
    r64, r32, _, _ = cs.bf16_pair(w, blocks)
    bar = 4 * nn_ref.distance(r32, r64)
    with Engine(games=len(st), sims=1, blocks=blocks, evaluator=_abi.EVAL_NN, precision=_abi.BF16) as e:
        e.load_weights(w)
        d = nn_ref.distance(e.nn_forward(st), r64)
        assert e.nn_fallbacks() == 0
    print(f"NNREF {tag} BF16: distance {d:.3e} bar {bar:.3e}")
    assert d <= bar


@pytest.mark.parametrize("name", sorted(cs.DEEP))
def test_bf16_at_depth_within_reference_noise(name):
    _bf16_by_noise_bar(f"c {name}", cs.deep_net(name), cs.DEEP[name])


@pytest.mark.parametrize("precision", sorted(NAMES))
def test_value_head_spread(precision):
    w = cs.value_net(precision)
    if precision == _abi.BF16:
        return _bf16_by_noise_bar("d", w, 3)
    st = np.array(cs.positions())
    ref = nn_ref.forward(w, 3, cs.planes())
    with Engine(games=len(st), sims=1, blocks=3, evaluator=_abi.EVAL_NN, precision=precision) as e:
        e.load_weights(w)
        d = nn_ref.distance(e.nn_forward(st), ref)
        assert e.nn_fallbacks() == 0
    print(f"NNREF d {NAMES[precision]}: distance {d:.3e} bar {cs.FP32_BARS[precision]:.0e}")
    assert d <= cs.FP32_BARS[precision]
