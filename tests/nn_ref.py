"""A plain float64 restatement of the network forward: TEST INFRASTRUCTURE ONLY (numpy only).

The op graph is net.rs's (ConvResNet::forward, train=false): conv_init_1 + bn1 + ReLU, `blocks`
residual blocks (conv + BN + ReLU, conv + BN, + skip, ReLU), the value head (1x1 conv + BN + ReLU,
linear 25 -> 64 + ReLU, linear 64 -> 1, tanh) and the policy head (1x1 conv to 2 planes + BN + ReLU,
linear 50 -> 50, softmax). Convolutions are im2col + matmul; nothing is fused and nothing is taken
from the kernels. BN is folded into the conv exactly as the packer folds it (oaz_pack.cpp fold():
s = g / sqrt(var + 1e-5) in double, w s and (b - mean) s + beta in double, then cast to float32), so
the folded weights are bit-equal to what the kernels consume.

Two modes:
  exact  no quantisation anywhere.
  bf16   the rounding points of the OAZ_BF16 kernel (k_nn_h3<H3Cfg<1>>) as its code states them:
           - first layer: folded fp32 weights, unquantised (the fp16 hi + lo first layer is exact to
             fp32 level); + bias, ReLU; the result is the fp32 skip;
           - every 64 -> 64 conv: folded weights rounded to bf16, round to nearest even
             (oaz_pack.cpp f32_to_bf16, split());
           - the input activations of every 64 -> 64 conv and of the head 1x1 convs: bf16 RNE of the
             previous epilogue's value (h3t_pack_one, the BF branch);
           - the fp32 bias is added unscaled; the residual is added from the UNQUANTISED skip kept
             in registers (h3t_pack_one: `v += skip` before the pack), then ReLU;
           - head 1x1 convs: bf16 activations x bf16 RNE folded head weights (h3_heads, the BF
             branch; pack_head_frags), fp32 bias, ReLU;
           - head MLPs, softmax, tanh: unquantised.

acc: the type of every accumulation and every stored value (np.float64: the specification;
np.float32: numpy float32 matmuls, the reference's own measure of summation-order noise).
head_acc: the same for the head MLPs, softmax and tanh alone (default: acc).

defect: a planted error, used only by tests/test_nn_ref.py to prove that the GPU comparisons can
see it (DEFECTS below lists the forms).
"""
from __future__ import annotations

import numpy as np

from onitama_az.weights import named_from_blob

BN_EPS = 1e-5
NEAR_BOUNDARY = 2.0 ** -18  # relative distance to a bf16 rounding boundary that counts as "near"

# defect forms (conv index: 0 = the first layer, 1 + 2 i + j = small block j (0 / 1) of block i)
#   ("drop_tap", conv, square, tap)       one tap of one output square of one conv contributes nothing
#   ("swap_cin", conv, c1, c2)            two input channels of one conv swapped
#   ("swap_cout", conv, c1, c2)           two output channels of one conv swapped (weights and bias)
#   ("block_weights", i, j)               block i computes with block j's weights
#   ("skip_quantised",)                   bf16: the residual read back from its bf16 copy
#   ("truncate",)                         bf16: activations truncated, not rounded to nearest even
#   ("unquantised_w",)                    bf16: the 64 -> 64 weights left in fp32
#   ("unquantised_head_w",)               bf16: the head 1x1 conv weights left in fp32
#   ("drop_value_feature", square)        one of the 25 value features reads as 0
#   ("swap_policy_features", f1, f2)      two of the 50 policy features swapped
#   ("wrong_player_cards",)               encode(): the mover's cards taken from the other player
DEFECTS = ("drop_tap", "swap_cin", "swap_cout", "block_weights", "skip_quantised", "truncate", "unquantised_w",
           "unquantised_head_w", "drop_value_feature", "swap_policy_features", "wrong_player_cards")


def encode(states: np.ndarray, defect=None) -> np.ndarray:
    """The encoder (common/mod.rs get_bit_array, deck.rs get_player_cards) in numpy: planes 0-3 the
    bitboards pawns[0], kings[0], pawns[1], kings[1] (square i = bit 31 - i), 4 + c all ones for the
    mover's two cards, 20 all ones when blue moves. [B, 21, 5, 5] float32."""
    B = len(states)
    out = np.zeros((B, 21, 25), dtype=np.float32)
    sh = (31 - np.arange(25)).astype(np.uint32)
    for p, (f, k) in enumerate((("pawns", 0), ("kings", 0), ("pawns", 1), ("kings", 1))):
        out[:, p] = (states[f][:, k].astype(np.uint32)[:, None] >> sh) & 1
    col = states["to_move"].astype(np.int64)
    out[:, 20] = col[:, None]
    s0 = 2 * (col ^ 1 if defect is not None and defect[0] == "wrong_player_cards" else col)
    for k in range(2):
        out[np.arange(B), 4 + (states["cards"][np.arange(B), s0 + k] & 15)] = 1.0
    return out.reshape(B, 21, 5, 5)


def fold(named, conv: str, bn: str):
    """conv + BN (eval) folded as oaz_pack.cpp fold(): double arithmetic, float32 results."""
    w = named[f"{conv}|weight"].astype(np.float64)
    b = named[f"{conv}|bias"].astype(np.float64)
    g, beta, mean, var = (named[f"{bn}|{f}"].astype(np.float64) for f in ("weight", "bias", "running_mean",
                                                                          "running_var"))
    s = g / np.sqrt(var + BN_EPS)
    return (w * s.reshape(-1, 1, 1, 1)).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)


def bf16_rne(x) -> np.ndarray:
    """float32 values of x rounded to bf16, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def bf16_trunc(x) -> np.ndarray:
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def near_bf16_boundary(v: np.ndarray) -> np.ndarray:
    """True where v > 0 lies within NEAR_BOUNDARY (relative) of the midpoint of two neighbouring
    bf16 values, where a different summation order may legitimately round the other way."""
    m, _ = np.frexp(np.where(v > 0, v, 1.0).astype(np.float64))  # m in [0.5, 1): 8 significant bits = steps of 2^-8
    t = m * 256.0
    return (v > 0) & (np.abs(t - np.floor(t) - 0.5) < NEAR_BOUNDARY * t)


def im2col(x: np.ndarray) -> np.ndarray:
    """[B, C, 5, 5] -> [B, 25, C, 9]: tap t = 3 kr + kc reads square (r + kr - 1, c + kc - 1), zero off board."""
    B, C = x.shape[:2]
    xp = np.zeros((B, C, 7, 7), dtype=x.dtype)
    xp[:, :, 1:6, 1:6] = x
    cols = np.empty((B, 25, C, 9), dtype=x.dtype)
    for t in range(9):
        cols[:, :, :, t] = xp[:, :, t // 3:t // 3 + 5, t % 3:t % 3 + 5].reshape(B, C, 25).transpose(0, 2, 1)
    return cols


def conv3x3(x: np.ndarray, w: np.ndarray, b: np.ndarray, drop=None) -> np.ndarray:
    """x [B, Ci, 5, 5] (the accumulation type), w [Co, Ci, 3, 3], b [Co] -> [B, Co, 5, 5], padding 1."""
    B, Ci = x.shape[:2]
    cols = im2col(x)
    if drop is not None:
        cols[:, drop[0], :, drop[1]] = 0
    y = cols.reshape(B * 25, Ci * 9) @ w.reshape(len(w), Ci * 9).astype(x.dtype).T + b.astype(x.dtype)
    return y.reshape(B, 25, len(w)).transpose(0, 2, 1).reshape(B, len(w), 5, 5)


def forward(blob: np.ndarray, blocks: int, planes: np.ndarray, mode: str = "exact", acc=np.float64, head_acc=None,
            defect=None, info: dict = None, tower=None):
    """(policy [B, 2, 25], value [B]) in the accumulation type. info (a dict, optional) receives
    'acts' (the tower's activations as the next layer reads them, one [B, 64, 5, 5] per layer) and
    'near' ([B] bool: a pre-rounding activation near a bf16 rounding boundary; bf16 mode),
    'pre_tanh' [B] and 'logits' [B, 50] (the heads' outputs before tanh and softmax).
    tower: the last entry of an earlier run's 'acts' with the same weights and planes; the tower is
    then not computed again (for runs that differ in the heads alone)."""
    assert mode in ("exact", "bf16")
    named = named_from_blob(np.ascontiguousarray(blob, dtype=np.float32), blocks)
    bf = mode == "bf16"
    kind = defect[0] if defect is not None else None
    assert kind is None or kind in DEFECTS
    head_acc = acc if head_acc is None else head_acc
    B = len(planes)
    near = np.zeros(B, dtype=bool)
    acts = []

    def q_act(v):  # what the next conv reads
        if not bf:
            acts.append(v)
            return v
        near[:] |= near_bf16_boundary(v).reshape(B, -1).any(1)
        r = (bf16_trunc(v) if kind == "truncate" else bf16_rne(v)).astype(acc)
        acts.append(r)
        return r

    def q_w(w, head=False):
        if not bf or kind == ("unquantised_head_w" if head else "unquantised_w"):
            return w
        return bf16_rne(w)

    def conv(idx, x, w, b):
        w, b = w.copy(), b.copy()
        if kind in ("swap_cin", "swap_cout") and defect[1] == idx:
            c1, c2 = defect[2], defect[3]
            if kind == "swap_cin":
                w[:, [c1, c2]] = w[:, [c2, c1]]
            else:
                w[[c1, c2]], b[[c1, c2]] = w[[c2, c1]], b[[c2, c1]]
        drop = (defect[2], defect[3]) if kind == "drop_tap" and defect[1] == idx else None
        return conv3x3(x, w, b, drop)

    if tower is not None:
        a = np.asarray(tower).astype(acc)
    else:
        w, b = fold(named, "conv_init_1", "bn1")
        skip = np.maximum(conv(0, np.asarray(planes).astype(acc), w, b), 0)
        a = q_act(skip)
        if kind == "skip_quantised":
            skip = a
        for i in range(blocks):
            src = defect[2] if kind == "block_weights" and defect[1] == i else i
            p1, p2 = (f"resnet_{src}|resnet_small_block{j}" for j in (1, 2))
            w, b = fold(named, f"{p1}|small_block_conv", f"{p1}|small_block_bn")
            h = q_act(np.maximum(conv(1 + 2 * i, a, q_w(w), b), 0))
            w, b = fold(named, f"{p2}|small_block_conv", f"{p2}|small_block_bn")
            skip = np.maximum(conv(2 + 2 * i, h, q_w(w), b) + skip, 0)
            a = q_act(skip)
            if kind == "skip_quantised":
                skip = a
    # heads: the 1x1 convs read the stored activations
    x = a.reshape(B, 64, 25).transpose(0, 2, 1).reshape(B * 25, 64)
    w, b = fold(named, "vh_conv", "vh_bn")
    fv = np.maximum(x @ q_w(w, True).reshape(1, 64).astype(acc).T + b.astype(acc), 0).reshape(B, 25)
    w, b = fold(named, "policy_conv", "policy_bn")
    fp = np.maximum(x @ q_w(w, True).reshape(2, 64).astype(acc).T + b.astype(acc), 0).reshape(B, 25, 2)
    fp = fp.transpose(0, 2, 1).reshape(B, 50)  # flatten of [B, 2, 5, 5]
    if kind == "drop_value_feature":
        fv = fv.copy()
        fv[:, defect[1]] = 0
    if kind == "swap_policy_features":
        fp = fp.copy()
        fp[:, [defect[1], defect[2]]] = fp[:, [defect[2], defect[1]]]
    fv, fp = fv.astype(head_acc), fp.astype(head_acc)
    lin = lambda x, n: x @ named[f"{n}|weight"].astype(head_acc).T + named[f"{n}|bias"].astype(head_acc)
    u = lin(np.maximum(lin(fv, "vh_linear1"), 0), "vh_linear2").reshape(B)
    value = np.tanh(u)
    lg = lin(fp, "ph_linear2")
    e = np.exp(lg - lg.max(1, keepdims=True))
    policy = (e / e.sum(1, keepdims=True)).reshape(B, 2, 25)
    if info is not None:
        info["acts"], info["near"], info["pre_tanh"], info["logits"] = acts, near, u, lg
    return policy, value


def distance(a, b) -> float:
    """max |policy difference|, |value difference| of two (policy, value) results."""
    return float(max(np.abs(np.asarray(a[0], np.float64) - b[0]).max(), np.abs(np.asarray(a[1], np.float64) - b[1]).max()))


def per_position(a, b) -> np.ndarray:
    """The same distance per position, [B]."""
    B = len(a[1])
    dp = np.abs(np.asarray(a[0], np.float64).reshape(B, 50) - np.asarray(b[0], np.float64).reshape(B, 50)).max(1)
    return np.maximum(dp, np.abs(np.asarray(a[1], np.float64).reshape(B) - np.asarray(b[1], np.float64).reshape(B)))
