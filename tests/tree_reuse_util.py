"""Tree reuse predicted from the unchanged oracle alone (tests/test_tree_reuse.py, tests/test_gpu_tree_reuse.py).
Needs no GPU. The rules restated here are the issue's, not the engine's code: the keep rule, the pass, the
last-maximum-of-visits move and the self-play loop whose ply p searches kept + sims playouts."""
import numpy as np

from conftest import random_positions
from onitama_az import _abi

NODE_FIELDS = ("W", "P", "N", "first", "mv", "nch", "flags", "pad")


def unpack(mv):
    """Packed oaz_node.mv -> (from, to, piece, slot)."""
    mv = int(mv)
    return (mv & 31, (mv >> 5) & 31, (mv >> 12) & 1, (mv >> 10) & 3)


def mv_tuple(m):
    return tuple(int(m[k]) for k in ("from_", "to", "piece", "slot"))


def stepped(orc, s, mv):
    """(position after the move or pass `mv` with the side to move flipped, MoveResult)."""
    s = s.reshape(1).copy()
    if mv[0] >= 25:  # pass (state.rs:139-142): the named card goes round with the neutral one
        c = s["cards"][0].copy()
        c[mv[3]], c[4] = c[4], c[mv[3]]
        s["cards"][0] = c
        res = _abi.IN_PROGRESS
    else:
        res = orc.make_move(s, mv, int(s["to_move"][0]))
    s["to_move"][0] ^= 1
    return s, res


def usable_roots(orc, n, seed):
    """n positions that are not won and have a child whose move does not win (the invariant's domain)."""
    out = []
    for r in random_positions(orc, 2 * n + 8, seed=seed):
        r = r.reshape(1)
        if orc.current_state(r) in (1, 2):
            continue
        if all(stepped(orc, r, mv_tuple(m))[1] in (1, 2) for m in orc.movegen(r)):
            continue
        out.append(r)
    assert len(out) >= n
    return np.concatenate(out[:n])


def assert_trees_equal(got, ref):
    """test_gpu._compare_trees' rule: every field, `first` only where the node is expanded; pad too."""
    assert len(got) == len(ref), (len(got), len(ref))
    for f in NODE_FIELDS:
        a, b = got[f], ref[f]
        if f == "first":
            a, b = np.where(got["flags"] & 1, a, 0), np.where(ref["flags"] & 1, b, 0)
        assert np.array_equal(a, b), f


def children(tree):
    root = tree[0]
    k = int(root["nch"]) if root["flags"] & 1 else 0
    return tree[int(root["first"]):int(root["first"]) + k]


def best_child(tree):
    """The last maximum of N among the root's children (mcts_arena.rs:87-94), or None without a child."""
    kids = children(tree)
    if len(kids) == 0:
        return None
    n = kids["N"].astype(np.int64)
    return int(len(n) - 1 - np.argmax(n[::-1]))


def least_visited_child(tree):
    kids = children(tree)
    seen = [k for k in range(len(kids)) if kids[k]["N"] >= 1]
    return min(seen, key=lambda k: (int(kids[k]["N"]), k))


def kept_visits(orc, tree, pos, k, sims_cap, R):
    """The keep rule: the N of the root's k-th child when its subtree is kept, else 0."""
    root, ch = tree[0], children(tree)[k]
    _, res = stepped(orc, pos, unpack(ch["mv"]))
    keep = (root["flags"] & 1) and (ch["flags"] & 1) and not (ch["flags"] & 2) and res not in (1, 2) and \
        int(ch["N"]) + sims_cap <= R
    return int(ch["N"]) if keep else 0


def fresh_search(orc, pos, sims, c_puct):
    """(move, pi [2, 25], tree) of the oracle's search from scratch."""
    mv, pi, nodes, _ = orc.search(orc.search_cfg(sims=sims, c_puct=c_puct, evaluator=orc.EVAL_HASH), pos)
    return mv, pi, nodes


def predicted_selfplay_game(orc, game_id, sims, c_puct, R, max_plies, seed, deck=None):
    """The samples of one self-play game with tree reuse, from orc.search alone: ply 0 searches `sims`
    playouts, each later ply kept + sims, kept = the played child's N in the previous ply's tree when the keep
    rule holds (R = 0: never). Returns (samples, plies whose search began on a kept tree, on a fresh one)."""
    s = orc.initial_state(deck if deck is not None else orc.deal_deck(seed, game_id))
    out, kept, n_kept, n_fresh = [], 0, 0, 0
    res = _abi.IN_PROGRESS
    for ply in range(max_plies + 2):
        n_kept, n_fresh = n_kept + (kept > 0), n_fresh + (kept == 0)
        _, pi, tree = fresh_search(orc, s, kept + sims, c_puct)
        rec = np.zeros(1, dtype=_abi.SAMPLE_DTYPE)
        rec["state"][0], rec["pi"][0] = s[0], pi.reshape(-1)
        out.append(rec)
        k = best_child(tree)
        if k is None:  # no legal move: pass with the mover's first card (Q6)
            mv, kept = (25, 25, 0, 2 if int(s["to_move"][0]) else 0), 0
        else:
            mv = unpack(children(tree)[k]["mv"])
            kept = kept_visits(orc, tree, s, k, sims, R) if R else 0
        s, res = stepped(orc, s, mv)
        if res in (1, 2):
            break
    out = np.concatenate(out)
    red_moved = out["state"]["to_move"] == 0  # z = reward(result, mover) (train.rs:83-85), 0 at the ply cut
    out["z"] = np.where((res == 1) == red_moved, 1.0, -1.0) if res in (1, 2) else 0.0
    return out, n_kept, n_fresh


def sorted_rows(a):
    """test_gpu._sorted_rows: the records as sorted byte rows."""
    return np.sort(np.frombuffer(a.tobytes(), dtype=np.dtype((np.void, a.dtype.itemsize))))
