"""Shared by tests/test_leaf_batch.py and tests/test_gpu_leaf_batch.py: the roots of the cases and the comparison of
an engine's dumped tree with the Python rule (tests/leaf_batch_ref.py)."""
import math

import numpy as np

import leaf_batch_ref as lbr
from onitama_az import _abi

C_PUCTS = (5.0, math.sqrt(2.0))
DECK = [0, 1, 2, 3, 4]  # Tiger Dragon | Frog Rabbit | Crab


def _bit(sq):
    return 1 << (31 - sq)


def start_root(orc, color):
    s = orc.initial_state(DECK)
    s["to_move"][0] = color
    return s


def sparse_endgame(color=0):
    """Two kings and a pawn each; Red's Tiger takes the blue king at once (17 -> 7), so a round's walks keep
    ending on the same won, terminal-flagged leaf."""
    a = np.zeros(1, dtype=_abi.STATE_DTYPE)
    a["kings"][0] = [_bit(17), _bit(7)]
    a["pawns"][0] = [_bit(21), _bit(3)]
    a["cards"][0] = DECK
    a["to_move"][0] = color
    return a


def midgame_roots(orc, n=3, seed=4245):
    """n distinct mid-game positions taken from one seeded random playout (plies 6, 9, 12, ..: both movers)."""
    import random
    rng = random.Random(seed)
    s = orc.initial_state(DECK)
    out = []
    for ply in range(6 + 3 * n):
        if ply >= 6 and (ply - 6) % 3 == 0:
            out.append(s.copy())
        moves = orc.movegen(s)
        assert len(moves) > 0
        m = moves[rng.randrange(len(moves))]
        r = orc.make_move(s, tuple(int(m[k]) for k in ("from_", "to", "piece", "slot")), int(s["to_move"][0]))
        assert r not in (1, 2)
        s["to_move"][0] ^= 1
    out = np.concatenate(out[:n])
    assert len({o.tobytes() for o in out}) == n
    return out


def kat_root(kats, name, color):
    from conftest import kat_state
    case = [c for c in kats["movegen"] if name in c["src"]][0]
    return kat_state(case["state"], color)


def ref_search(root, sims, c, L, evaluator=lbr.hash_eval):
    """(move tuple (from, to, piece, slot) with the engine's pass move for a root without a child, pi float32 [50],
    nodes NODE_DTYPE, (rounds, discarded))."""
    gs = lbr.state_of(root)
    mv, pi, arena, rd = lbr.search(gs, sims, c, L, evaluator)
    move = (mv[1], mv[2], mv[3], mv[0]) if mv is not None else (25, 25, 0, 2 * gs.color)
    return move, np.array(pi, dtype=np.float32), lbr.arena_nodes(arena, _abi.NODE_DTYPE), rd


def assert_tree_equals(t, ref):
    """Index for index: N, W and P as f64 bit patterns, first (where the node has children), nch, mv, flags, and
    every in-flight count back at 0."""
    assert len(t) == len(ref), (len(t), len(ref))
    assert np.array_equal(t["N"], ref["N"])
    for f in ("W", "P"):
        assert np.array_equal(t[f].view(np.uint64), ref[f].view(np.uint64)), f
    kids = ref["nch"] > 0
    assert np.array_equal(t["nch"], ref["nch"]) and np.array_equal(t["first"][kids], ref["first"][kids])
    assert np.array_equal(t["mv"], ref["mv"]) and np.array_equal(t["flags"], ref["flags"])
    assert not t["pad"].any() and not ref["pad"].any()
