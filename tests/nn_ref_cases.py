"""Inputs and networks shared by tests/test_nn_ref.py (CPU: the conditions on them) and
tests/test_gpu_nn_ref.py (GPU: the comparisons) — TEST INFRASTRUCTURE ONLY. Everything is generated
from seeds; nothing here touches the GPU library."""
from __future__ import annotations

import functools

import numpy as np

import nn_ref
from onitama_az import _abi
from onitama_az.weights import blob_from_named, canonical_layout

DEPTHS_A = (0, 1, 2, 3, 5, 6)
SEEDS_A_BY_DEPTH = {d: (1, 2, 3) for d in DEPTHS_A}  # integer nets per depth
DEPTHS_B = (0, 1)
SEEDS_B = (11, 12)

# The bars (tests/test_nn_ref.py re-measures the distances on the CPU and holds the constants to them).
# (a): the largest distance, over the 18 integer nets and positions(), between the float64 reference and
# the same reference with the head MLPs, softmax and tanh in float32: measured 4.59e-7 (depth 1, seed 1;
# 2.1e-7 to 4.6e-7 per depth). The device's expf / tanhf and summation order differ from both: 8x.
A_DIST = 4.6e-7
BAR_A = 8 * A_DIST
# (b): the largest distance between the bf16-mode reference with float64 and with float32 accumulation
# everywhere, over the shallow nets, on the positions where both runs round every activation the same
# way: measured 4.16e-8 (depth 0), 1.42e-8 (depth 1). Where a rounding differs the distance is that of
# one bf16 ulp (3.5e-6 to 6.2e-5), which is what the exclusion rule is for. 8x, and (a)'s bar as the floor
# (the heads are the same fp32 code).
B_DIST = 4.2e-8
BAR_B = max(BAR_A, 8 * B_DIST)
EXCLUDE_CAP = 0.02  # (b): at most this share of the positions may lie beyond the bar, each near a bf16 boundary
FP32_BARS = {_abi.FP32: 1e-4, _abi.FP32_SPLIT: 1e-4, _abi.FP32_SPLIT16: 1e-5}  # (d): the project's fp32-level bars


# ---- positions -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def positions() -> np.ndarray:
    """150 positions of random play (both colours, all phases), 100 one-hot boards (one piece of one
    bitboard on each square, the other boards empty) and 64 positions that give the mover each of
    the 16 cards in each of its two slots, for both colours: 314 = 19 x 16 + 10 states. nn_forward
    needs no legal position."""
    import oracle_ffi as orc
    from conftest import random_positions
    rnd = random_positions(orc, 150, seed=20261020)
    hot = np.zeros(100, dtype=_abi.STATE_DTYPE)
    for b, (f, k) in enumerate((("kings", 0), ("kings", 1), ("pawns", 0), ("pawns", 1))):
        for sq in range(25):
            s = hot[b * 25 + sq:b * 25 + sq + 1]
            s[f][0, k] = np.uint32(1) << np.uint32(31 - sq)
            s["cards"][0] = [(sq + b + j * 3) % 16 for j in range(5)]
            s["to_move"][0] = (sq + b) & 1
    cards = np.zeros(64, dtype=_abi.STATE_DTYPE)
    n = 0
    for colour in (0, 1):
        for slot in (0, 1):
            for c in range(16):
                s = cards[n:n + 1]
                s[0] = rnd[n]
                rest = [(c + 1 + 3 * j) % 16 for j in range(4)]  # distinct, never c
                deck = np.zeros(5, dtype=np.uint8)
                deck[2 * colour + slot] = c
                deck[[i for i in range(5) if i != 2 * colour + slot]] = rest
                s["cards"][0], s["to_move"][0] = deck, colour
                n += 1
    out = np.concatenate([rnd, hot, cards])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planes() -> np.ndarray:
    """The oracle's encoding of positions() (orc_encode), [314, 21, 5, 5]."""
    import oracle_ffi as orc
    st = positions()
    out = np.stack([orc.encode(st[i]) for i in range(len(st))])
    out.setflags(write=False)
    return out


# ---- networks ------------------------------------------------------------------------------------
def _is_bn(name):
    return name.split("|")[-2].endswith(("bn", "bn1"))


def random_net(seed: int, blocks: int) -> np.ndarray:
    """Ordinary weights: U(+-1/sqrt(fan_in)) convs and linears, BN away from the identity (gamma in
    [0.7, 1.3], beta and mean in +-0.2, var in [0.5, 1.5]) so that the fold is exercised."""
    rng = np.random.default_rng([seed, blocks, 77])
    named, fan = {}, 1
    for name, shape in canonical_layout(blocks):
        f = name.split("|")[-1]
        if _is_bn(name):
            lo, hi = {"weight": (0.7, 1.3), "bias": (-0.2, 0.2), "running_mean": (-0.2, 0.2),
                      "running_var": (0.5, 1.5)}[f]
            named[name] = rng.uniform(lo, hi, shape)
        else:
            if f == "weight":
                fan = int(np.prod(shape[1:]))
            named[name] = rng.uniform(-1, 1, shape) / np.sqrt(fan)
    return blob_from_named({k: v.astype(np.float32) for k, v in named.items()}, blocks)


def _spread_heads(named, blocks, mode="exact", span=1.6, logit_range=2.0):
    """Scale vh_linear2 and ph_linear2 (in place) on the reference's own run over planes(): the
    value's pre-tanh output then spans `span` around 0 and the widest policy row's logits span
    `logit_range`, so value covers most of (-1, 1) and the policy rows differ without saturating."""
    named["vh_linear2|bias"] = np.zeros(1, dtype=np.float32)
    info = {}
    nn_ref.forward(blob_from_named(named, blocks), blocks, planes(), mode=mode, info=info)
    u, lg = info["pre_tanh"], info["logits"]
    k = span / (u.max() - u.min())
    named["vh_linear2|weight"] = (named["vh_linear2|weight"] * k).astype(np.float32)
    named["vh_linear2|bias"] = np.array([-k * (u.max() + u.min()) / 2], dtype=np.float32)
    kp = logit_range / (lg.max(1) - lg.min(1)).max()
    named["ph_linear2|weight"] = (named["ph_linear2|weight"] * kp).astype(np.float32)
    named["ph_linear2|bias"] = (named["ph_linear2|bias"] * kp).astype(np.float32)


def _sparse_conv(rng, cin, cov_in, cov_out, per_out=3):
    """[64, cin, 3, 3] of 0 / +-1 with per_out nonzeros per output channel, placed first on the
    (tap, input channel) and (tap, output channel) pairs that no earlier layer sharing cov_in /
    cov_out has used, so that a few layers together carry a weight on every such pair."""
    w = np.zeros((64, cin, 9), dtype=np.float32)
    for co in rng.permutation(64):
        for _ in range(per_out):
            taps = np.nonzero(~cov_out[:, co])[0]
            taps = taps if len(taps) else np.arange(9)
            t = int(taps[np.argmax((~cov_in[taps]).sum(1) + rng.random(len(taps)))])
            cis = np.nonzero(~cov_in[t])[0]
            ci = int(rng.choice(cis if len(cis) else np.arange(cin)))
            w[co, ci, t] = rng.choice([-1.0, 1.0])
            cov_in[t, ci] = cov_out[t, co] = True
    return w.reshape(64, cin, 3, 3)


@functools.lru_cache(maxsize=None)
def integer_nets(depth: int):
    """The exact-integer nets of one depth, one blob per seed of SEEDS_A_BY_DEPTH[depth]: sparse +-1 tower
    weights, integer biases (0 / 1; -1 on each block's second conv), BN that folds to exactly 1
    (var = 1 - 1e-5), head 1x1 convs of +-1/8 and bias 1/2: every tower activation is a small
    integer and every head feature a multiple of 1/8, which all four precisions represent and sum
    exactly. Only the fp32 head MLPs, softmax and tanh are left to differ from float64."""
    cov = {k: np.zeros((9, n), dtype=bool) for k, n in (("in", 64), ("out", 64), ("pl", 21), ("o1", 64))}
    ident = {"weight": 1.0, "bias": 0.0, "running_mean": 0.0, "running_var": np.float32(1.0 - 1e-5)}
    out = []
    for seed in SEEDS_A_BY_DEPTH[depth]:
        rng = np.random.default_rng([seed, depth, 20261020])
        named = {}
        for name, shape in canonical_layout(depth):
            f = name.split("|")[-1]
            if _is_bn(name):
                named[name] = np.full(shape, ident[f], dtype=np.float32)
            elif name == "conv_init_1|weight":
                named[name] = _sparse_conv(rng, 21, cov["pl"], cov["o1"])
            elif name.endswith("small_block_conv|weight"):
                named[name] = _sparse_conv(rng, 64, cov["in"], cov["out"])
            elif name.endswith("small_block_conv|bias"):
                named[name] = np.full(shape, -1.0) if "small_block2" in name else rng.integers(0, 2, shape)
            elif name == "conv_init_1|bias":
                named[name] = rng.integers(0, 2, shape)
            elif name in ("vh_conv|weight", "policy_conv|weight"):
                named[name] = rng.choice([-0.125, 0.0, 0.0, 0.125], shape)
            elif name in ("vh_conv|bias", "policy_conv|bias"):
                named[name] = np.full(shape, 0.5)
            else:  # the head MLPs: ordinary weights, scaled below
                fan = shape[-1]
                named[name] = rng.uniform(-1, 1, shape) / np.sqrt(fan)
        named = {k: np.asarray(v, dtype=np.float32) for k, v in named.items()}
        _spread_heads(named, depth)
        out.append(blob_from_named(named, depth))
    return tuple(out)


def integer_runs(depth: int):
    """The exact reference on planes() for each net of integer_nets(depth): yields ((policy, value),
    the tower's activations per layer)."""
    for w in integer_nets(depth):
        info = {}
        yield nn_ref.forward(w, depth, planes(), info=info), info["acts"]


@functools.lru_cache(maxsize=None)
def integer_refs(depth: int):
    """The exact reference's (policy, value) on planes() for each net of integer_nets(depth)."""
    return tuple(nn_ref.forward(w, depth, planes()) for w in integer_nets(depth))


@functools.lru_cache(maxsize=None)
def shallow_nets(depth: int):
    """(b): ordinary random nets of depth 0 / 1, one per seed of SEEDS_B."""
    return tuple(random_net(seed, depth) for seed in SEEDS_B)


# (d): seeds whose value head is alive before the scaling (of the seeds 40-51 four give a value conv whose
# ReLU is zero on every position; scaling such a head up would only amplify rounding noise)
VALUE_SEEDS = {_abi.FP32: 43, _abi.BF16: 46, _abi.FP32_SPLIT: 48, _abi.FP32_SPLIT16: 44}
DEEP = {"trained3": 3, "trained5": 5, "random6": 6}  # (c)


@functools.lru_cache(maxsize=None)
def deep_net(name: str):
    from conftest import GOLDEN
    if name == "random6":
        return random_net(21, 6)
    return np.load(GOLDEN / f"weights_{DEEP[name]}block_trained.npy", allow_pickle=False)


@functools.lru_cache(maxsize=None)
def value_net(precision: int):
    """(d): 3 blocks, ordinary weights, the value head's last layer scaled and biased so that value
    covers most of (-1, 1) over positions(); one net per precision."""
    from onitama_az.weights import named_from_blob
    named = {k: v.copy() for k, v in named_from_blob(random_net(VALUE_SEEDS[precision], 3), 3).items()}
    _spread_heads(named, 3)
    return blob_from_named(named, 3)


# ---- the reference's runs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes_wrong_cards() -> np.ndarray:
    return nn_ref.encode(positions(), ("wrong_player_cards",))


def bf16_pair(blob, blocks):
    """The bf16-mode reference with float64 and with float32 accumulation: (r64, r32, near [B],
    same [B]: every stored activation of the position rounded the same way in both runs)."""
    i64, i32 = {}, {}
    r64 = nn_ref.forward(blob, blocks, planes(), mode="bf16", info=i64)
    r32 = nn_ref.forward(blob, blocks, planes(), mode="bf16", acc=np.float32, info=i32)
    same = np.ones(len(planes()), dtype=bool)
    for a, b in zip(i64["acts"], i32["acts"]):
        same &= (a.astype(np.float32) == b.astype(np.float32)).reshape(len(same), -1).all(1)
    return r64, r32, i64["near"], same


def defects(blocks: int):
    """The planted defects that exist at this depth, on the last conv of the tower."""
    last = 2 * blocks
    c = (1, 3) if blocks == 0 else (5, 37)  # the first layer has 21 input planes: the two kings' planes
    out = [("drop_tap", last, 0, 8), ("swap_cin", last, *c), ("swap_cout", last, 5, 37), ("drop_value_feature", 7),
           ("swap_policy_features", 3, 30), ("wrong_player_cards",), ("truncate",), ("unquantised_head_w",)]
    if blocks >= 1:
        out += [("skip_quantised",), ("unquantised_w",)]
    if blocks >= 2:
        out += [("block_weights", 0, blocks - 1)]
    return out


ROUNDING_DEFECTS = ("truncate", "unquantised_head_w", "skip_quantised", "unquantised_w")  # bf16 mode only


def moved_by(defect, blob, blocks, mode, base) -> np.ndarray:
    """Per position, how far the defect moves the reference from its own sound run `base`."""
    pl = planes_wrong_cards() if defect[0] == "wrong_player_cards" else planes()
    return nn_ref.per_position(nn_ref.forward(blob, blocks, pl, mode=mode, defect=defect), base)
