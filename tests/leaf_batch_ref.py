"""The leaf-parallel search rule (oaz_config.leaf_batch, DESIGN.md "Leaf-parallel search") in pure Python —
TEST INFRASTRUCTURE, written from the specification of the rule, not from the kernel.

leaf_batch = L, 1 <= L <= 16. Every node has an in-flight count v (0 outside a round). A search of `sims`
playouts proceeds in rounds until done == sims:

  collect   for j = 0 .. min(L, sims - done) - 1, in this order: walk from the root as pyref.search does, on the
            effective statistics of child c under parent p
                n = N_c + v_c,  q = (W_c - float(v_c)) / float(n) if n else 0.0,
                u = q + c_puct * P_c * (sqrt(float(N_p + v_p)) / float(n + 1)),
            the last maximum winning, a child whose move wins flagged terminal. The walk stops on an unexpanded,
            terminal-flagged or stuck (no children) node. If that node is neither expanded nor terminal-flagged
            and has v > 0, the walk is discarded (no virtual loss, no playout; terminal flags it set stay) and
            the round closes. Otherwise v += 1 on every node of the path, root included, and the path and the
            leaf position are leaf j.
  evaluate  the m collected leaf positions together.
  back up   for j = 0 .. m - 1, in order: v -= 1 along path j, then pyref.search's expand / back up of that
            playout unchanged (node indices are allocated in order j). done += m.

The rules and the HASH evaluator come from tests/pyref.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from pyref import Node, S, _f32, _key, current_state, hash_eval, legal_moves, make_move


@dataclass
class VNode(Node):
    v: int = 0  # playouts in flight through this node


def _reward(res, color):
    if res == 1:
        return 1.0 if color == 0 else -1.0
    if res == 2:
        return 1.0 if color == 1 else -1.0
    return 0.0


def search(root: S, sims: int, c: float, leaf_batch: int, evaluator=hash_eval):
    """Returns (move, pi[50], arena, (rounds, discarded walks))."""
    assert 1 <= leaf_batch <= 16 and sims >= 1
    arena = [VNode(None, None, root.color, 1.0)]
    done = rounds = discarded = 0
    while done < sims:
        leaves = []
        for _ in range(min(leaf_batch, sims - done)):
            gs = root.copy()
            node, path = 0, [0]
            while arena[node].expanded and not arena[node].terminal:
                p = arena[node]
                if not p.children:  # stuck (Q6): a leaf
                    break
                sq = math.sqrt(float(p.visits + p.v))
                best, bk = None, None
                for ci in p.children:
                    ch = arena[ci]
                    n = ch.visits + ch.v
                    q = (ch.reward - float(ch.v)) / float(n) if n else 0.0
                    u = q + c * ch.prob * (sq / float(n + 1))
                    k = _key(u)
                    if best is None or not (bk > k):
                        best, bk = ci, k
                node = best
                res = make_move(gs, arena[node].mov, p.color)
                gs.color ^= 1
                if res in (1, 2):
                    arena[node].terminal = True
                path.append(node)
            nd = arena[node]
            if not nd.expanded and not nd.terminal and nd.v > 0:  # collision: the round closes
                discarded += 1
                break
            for i in path:
                arena[i].v += 1
            leaves.append((path, gs))
        evals = [evaluator(gs) for _, gs in leaves]
        for (path, gs), (pol, val) in zip(leaves, evals):
            for i in path:
                arena[i].v -= 1
            node = path[-1]
            moves = legal_moves(gs, gs.color)
            pri = [[0.0] * 25, [0.0] * 25]
            for (slot, fr, to, piece) in moves:
                pri[slot % 2][to] = float(pol[(slot % 2) * 25 + to])
            for r in range(2):
                tot = 0.0
                for x in pri[r]:
                    tot += x
                if tot > 0.0:
                    pri[r] = [x / tot for x in pri[r]]
            if not arena[node].expanded and not arena[node].terminal:
                for mv in moves:
                    arena.append(VNode(node, mv, arena[node].color ^ 1, pri[mv[0] % 2][mv[2]]))
                    arena[node].children.append(len(arena) - 1)
                arena[node].expanded = True
            parent = arena[node].parent if arena[node].parent is not None else 0
            mr = current_state(gs)
            r = _reward(mr, arena[parent].color) if mr in (1, 2) else float(val)
            for i in reversed(path):
                arena[i].visits += 1
                arena[i].reward += r
                r = -r
        done += len(leaves)
        rounds += 1
    rootn = arena[0]
    pi = [0.0] * 50
    for ci in rootn.children:
        ch = arena[ci]
        pi[(ch.mov[0] % 2) * 25 + ch.mov[2]] += ch.visits
    tot = _f32(sum(pi))
    pi = [_f32(_f32(x) / tot) if tot > 0 else 0.0 for x in pi]
    best = None
    for ci in rootn.children:
        if best is None or not (arena[best].visits / rootn.visits > arena[ci].visits / rootn.visits):
            best = ci
    return (arena[best].mov if best is not None else None), pi, arena, (rounds, discarded)


def state_of(s) -> S:
    """A STATE_DTYPE record as the reference's state."""
    s = np.asarray(s).reshape(1)
    return S(list(map(int, s["kings"][0])), list(map(int, s["pawns"][0])), list(map(int, s["cards"][0])),
             int(s["to_move"][0]))


def state_np(gs: S, dtype):
    a = np.zeros(1, dtype=dtype)
    a["kings"][0], a["pawns"][0], a["cards"][0], a["to_move"][0] = gs.kings, gs.pawns, gs.cards, gs.color
    return a


def arena_nodes(arena, dtype):
    """The arena as the engine dumps a tree (NODE_DTYPE): children contiguous from `first` (0 without children),
    mv = from | to << 5 | slot << 10 | piece << 12, flags bit 0 expanded, bit 1 terminal, pad = v."""
    out = np.zeros(len(arena), dtype=dtype)
    for i, nd in enumerate(arena):
        out["W"][i], out["P"][i], out["N"][i] = nd.reward, nd.prob, nd.visits
        if nd.children:
            assert nd.children == list(range(nd.children[0], nd.children[0] + len(nd.children)))
            out["first"][i] = nd.children[0]
        out["nch"][i] = len(nd.children)
        if nd.mov is not None:
            slot, fr, to, piece = nd.mov
            out["mv"][i] = fr | to << 5 | slot << 10 | piece << 12
        out["flags"][i] = (1 if nd.expanded else 0) | (2 if nd.terminal else 0)
        out["pad"][i] = nd.v
    return out
