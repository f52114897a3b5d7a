"""The held-out split and the eval-mode statistics restated (include/onitama_az.h, "held-out evaluation"): what
tests/test_holdout.py and tests/test_gpu_train_eval.py compare oaz_holdout_* and oaz_trainer_evaluate / predict
with. Written from the rule's text: Philox4x32-10 spelled out on numpy uint64 arrays, the key from the record's
bytes, the statistics with numpy from oracle/train_ref.py's forward(train=False) in float64 (float32 on request:
the yardstick of tests/train_util.py, not a second oracle). Nothing here calls the library.
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from onitama_az import _abi
from onitama_az.weights import named_from_blob

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))

M32 = np.uint64(0xFFFFFFFF)
HOLD = 0x484F4C44  # "HOLD"


def philox(key, c0, c1, c2, c3):
    """Philox4x32-10: key uint64 [n] (low word k0, high word k1), four counter words; returns the four output
    words as uint64 arrays holding 32-bit values."""
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key & M32, key >> np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def key_words(samples):
    """[n, 6] uint64: the 22 key bytes of every record (kings[2], pawns[2], cards[5], to_move) as six little-endian
    32-bit words, the pad bytes 0."""
    st = np.ascontiguousarray(samples["state"] if "state" in (samples.dtype.names or ()) else samples)
    raw = np.frombuffer(st.tobytes(), dtype=np.uint8).reshape(len(st), 24).copy()
    raw[:, 22:] = 0
    return raw.view("<u4").astype(np.uint64)


def holdout_mask(samples, seed, per_65536):
    """uint8 [n]: a = philox(seed; k0..k3); b = philox(a.w0 | a.w1 << 32; k4, k5, "HOLD", 0);
    held out iff (b.w0 & 0xFFFF) < per_65536."""
    if len(samples) == 0:
        return np.zeros(0, dtype=np.uint8)
    k = key_words(samples)
    n = len(k)
    a = philox(np.full(n, seed, dtype=np.uint64), k[:, 0], k[:, 1], k[:, 2], k[:, 3])
    b = philox(a[0] | (a[1] << np.uint64(32)), k[:, 4], k[:, 5], np.full(n, HOLD, dtype=np.uint64),
               np.zeros(n, dtype=np.uint64))
    return ((b[0] & np.uint64(0xFFFF)) < np.uint64(per_65536)).astype(np.uint8)


def forward_eval(w, blocks, planes, dtype=np.float64, bn_eps=1e-5):
    """(p [n, 50], v [n]) of train_ref.forward(train=False) on the blob w, as numpy arrays of `dtype`."""
    import torch
    from train_ref import forward
    with torch.no_grad():
        p, v = forward(named_from_blob(np.asarray(w, dtype=np.float32), blocks), planes, blocks, train=False,
                       dtype=dtype, bn_eps=bn_eps)
    return p.numpy().reshape(-1, 50), v.numpy().reshape(-1)


def entries(orc, samples, idx=None, reflect=None):
    """The records an (idx, reflect) call evaluates, reflected ones as reflect_util-reflected records, and their
    encoded planes [n, 21, 5, 5] (the oracle's create_tensor_from_state)."""
    import reflect_util as ru
    rec = samples if idx is None else samples[np.asarray(idx)]
    rec = np.ascontiguousarray(rec).copy()
    if reflect is not None:
        f = np.asarray(reflect).astype(bool)
        if f.any():
            rec[f] = ru.reflect_samples(np.ascontiguousarray(rec[f]))
    states = np.ascontiguousarray(rec["state"])
    planes = np.stack([orc.encode(states[i:i + 1]) for i in range(len(rec))]) if len(rec) else np.zeros((0, 21, 5, 5))
    return rec, planes.reshape(len(rec), 21, 5, 5)


def stats(p, v, pi, z):
    """oaz_eval_stats from predictions and targets, in the arrays' precision: the sums, the counts, and per record
    the float64-side margins the count comparisons leave borderline records out by (gap: the top-two p gap;
    |v|)."""
    p, v = np.asarray(p), np.asarray(v)
    pi, z = np.asarray(pi).astype(p.dtype), np.asarray(z).astype(p.dtype)
    n = len(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        ce = -np.where(pi != 0, pi * np.log(p), 0).sum(1) if n else np.zeros(0)
        ent = -np.where(pi != 0, pi * np.log(np.where(pi != 0, pi, 1)), 0).sum(1) if n else np.zeros(0)
    am = p.argmax(1) if n else np.zeros(0, dtype=np.int64)  # numpy: the lowest index on ties
    top1 = pi[np.arange(n), am] == pi.max(1) if n else np.zeros(0, dtype=bool)
    decided = z != 0
    sign = decided & (v * z > 0)
    srt = np.sort(p, axis=1) if n else np.zeros((0, 50))
    return SimpleNamespace(n=n, decided=int(decided.sum()), top1=int(top1.sum()), sign=int(sign.sum()),
                           value_sq=float(((z - v) ** 2).sum()), policy_ce=float(ce.sum()),
                           target_entropy=float(ent.sum()), top1_each=top1, sign_each=sign, decided_each=decided,
                           gap=(srt[:, -1] - srt[:, -2]) if n else np.zeros(0), absv=np.abs(v))
