"""Playout cap randomization (oaz_selfplay_set_playout_cap) predicted from the unchanged oracle alone
(tests/test_playout_cap.py, tests/test_gpu_playout_cap.py). Needs no GPU. The rule restated here is the issue's, not
the engine's code: over orc.philox, in Python integers.

    ply `ply` of global game `gid` under `seed` is full  iff  (Philox(seed; gid lo, gid hi, TAG, ply)[0] >> 16) < P

A full ply is searched with `sims` playouts and recorded, a fast one with `n` and only played; both play the move the
engine would play from that tree (temperature_util.played_child)."""
import numpy as np

from onitama_az import _abi
from temperature_util import played_child, search_tree
from tree_reuse_util import children, stepped, unpack

TAG = 0x50434150  # "PCAP": Philox counter word 2 of a cap draw


def is_full(orc, seed, gid, ply, P):
    """Whether the ply is a full one when P of 65 536 are."""
    assert 0 <= P <= 65536
    w = int(orc.philox(seed, [gid & 0xFFFFFFFF, gid >> 32, TAG, ply])[0])
    return (w >> 16) < P


def budget(orc, seed, gid, ply, sims, n, P):
    """The playouts of the ply: `sims` on a full ply, `n` on a fast one."""
    return sims if is_full(orc, seed, gid, ply, P) else n


def predicted_selfplay_game(orc, game_id, sims, n, P, c_puct, max_plies, seed, T=0, deck=None, train_noise=0):
    """One capped self-play game from orc.search alone: a fresh search per ply with `sims` or `n` playouts by the
    rule, the temperature rule's child while ply < T, else the last maximum of the visits, the pass without a child.
    Returns (samples: the full plies' records in ply order, z filled in; moves: the move sequence as tuples;
    info = dict(full, fast: plies of each kind))."""
    s = orc.initial_state(deck if deck is not None else orc.deal_deck(seed, game_id))
    out, moves = [], []
    info = dict(full=0, fast=0)
    res = _abi.IN_PROGRESS
    for ply in range(max_plies + 2):
        full = is_full(orc, seed, game_id, ply, P)
        info["full" if full else "fast"] += 1
        pi, tree = search_tree(orc, s, sims if full else n, c_puct, seed, train_noise, game_id, ply)
        if full:
            rec = np.zeros(1, dtype=_abi.SAMPLE_DTYPE)
            rec["state"][0], rec["pi"][0] = s[0], pi.reshape(-1)
            out.append(rec)
        k, _ = played_child(orc, tree, seed, game_id, ply, T)
        if k is None:  # no legal move: pass with the mover's first card (Q6)
            mv = (25, 25, 0, 2 if int(s["to_move"][0]) else 0)
        else:
            mv = unpack(children(tree)[k]["mv"])
        moves.append(mv)
        s, res = stepped(orc, s, mv)
        if res in (1, 2):
            break
    out = np.concatenate(out) if out else np.zeros(0, dtype=_abi.SAMPLE_DTYPE)
    red_moved = out["state"]["to_move"] == 0  # z = reward(result, mover) (train.rs:83-85), 0 at the ply cut
    out["z"] = np.where((res == 1) == red_moved, 1.0, -1.0) if res in (1, 2) else 0.0
    return out, tuple(moves), info
