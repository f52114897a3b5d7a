"""The replay buffer's merge rule and window, restated in numpy and plain lists (include/onitama_az.h, "replay
buffer"): what tests/test_replay.py and tests/test_gpu_replay.py compare oaz_replay_* with. Written from the
rule's text: a dict of key bytes for the groups, Python integers for the sums, numpy float64 / float32 for the
two roundings. Nothing here calls the library.
"""
import numpy as np

from onitama_az import _abi

TWO32 = np.float64(4294967296.0)


def key_bytes(rec) -> bytes:
    """The 22 key bytes of one record: kings[2], pawns[2], cards[5], to_move (the state's first 22 bytes; pad is
    the last two)."""
    return rec["state"].tobytes()[:22]


def merge(samples):
    """(merged records, mult uint32): one record per group of equal key, in the order of each group's first
    member. A group of one is its record byte for byte; else the first member's state and, for the 50 pi entries
    and z, float32(float64(sum of rint(x * 2^32)) / (float64(m) * 2^32))."""
    samples = np.ascontiguousarray(samples, dtype=_abi.SAMPLE_DTYPE)
    groups = {}  # key -> member indices in arrival order (dicts keep the order of first insertion)
    for i in range(len(samples)):
        groups.setdefault(key_bytes(samples[i]), []).append(i)
    out = np.zeros(len(groups), dtype=_abi.SAMPLE_DTYPE)
    mult = np.zeros(len(groups), dtype=np.uint32)
    for g, members in enumerate(groups.values()):
        m = len(members)
        mult[g] = m
        out[g] = samples[members[0]]
        if m == 1:
            continue
        fixed_pi = np.rint(samples["pi"][members].astype(np.float64) * TWO32)  # [m, 50], integers in float64: exact
        fixed_z = np.rint(samples["z"][members].astype(np.float64) * TWO32)
        for j in range(50):
            s = sum(int(v) for v in fixed_pi[:, j])
            out["pi"][g, j] = np.float32(np.float64(s) / (np.float64(m) * TWO32))
        s = sum(int(v) for v in fixed_z)
        out["z"][g] = np.float32(np.float64(s) / (np.float64(m) * TWO32))
    return out, mult


def window(appends, window_segments, capacity):
    """What the window holds after `appends` (a list of record arrays, one per segment, oldest first): the list
    of surviving segments. A segment larger than capacity is refused (skipped, as the caller sees an error)."""
    segs = []
    for a in appends:
        if len(a) > capacity:
            continue
        segs.append(a)
        while len(segs) > window_segments:
            segs.pop(0)
        while sum(len(s) for s in segs) > capacity and len(segs) > 1:
            segs.pop(0)
    return segs


def concat(segs):
    return np.concatenate(segs) if segs else np.zeros(0, dtype=_abi.SAMPLE_DTYPE)


Z_VALUES = (-1.0, 0.0, 1.0, 0.5, -0.25)


def synthetic(key_ids, seed):
    """One record per entry of key_ids, the key a function of the id (kings[0] = (id + 1) << 7, a card, the
    colour): sparse normalised random pi, z drawn from Z_VALUES, random pad bytes. The states are not positions
    of the game; the merge does not look."""
    key_ids = np.asarray(key_ids, dtype=np.int64)
    n = len(key_ids)
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=_abi.SAMPLE_DTYPE)
    rec["state"]["kings"][:, 0] = ((key_ids + 1) << 7) & 0xFFFFFFFF
    rec["state"]["pawns"][:, 1] = (key_ids * 0x9E3779B1) & 0xFFFFFF80
    rec["state"]["cards"] = np.array([0, 1, 2, 3, 4], dtype=np.uint8)
    rec["state"]["cards"][:, 0] = key_ids % 16
    rec["state"]["to_move"] = key_ids & 1
    rec["state"]["pad"] = rng.integers(0, 256, (n, 2))
    pi = rng.random((n, 50)) * (rng.random((n, 50)) < 0.3)
    pi[:, 0] += 1e-3
    rec["pi"] = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    rec["z"] = rng.choice(Z_VALUES, n).astype(np.float32)
    return rec


def mixed_ids(mults, seed):
    """Key ids 0 .. len(mults) - 1, id k repeated mults[k] times, shuffled."""
    ids = np.repeat(np.arange(len(mults)), mults)
    np.random.default_rng(seed).shuffle(ids)
    return ids
