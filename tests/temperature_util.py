"""Self-play temperature (oaz_config.temperature_plies) predicted from the unchanged oracle alone
(tests/test_temperature.py, tests/test_gpu_temperature.py). Needs no GPU. The rule restated here is the issue's,
not the engine's code: over orc.philox, in Python integers."""
import numpy as np

from onitama_az import _abi
from tree_reuse_util import best_child, children, kept_visits, stepped, unpack

TAG = 0x54454D50  # "TEMP": Philox counter word 2 of a temperature draw


def pick(orc, seed, gid, ply, visits):
    """The child the rule draws for (seed, game id, ply) from the root children's visits in node order, or None
    when it draws nothing (no child, or no visit)."""
    n = [int(v) for v in visits]
    S = sum(n) & 0xFFFFFFFF
    if len(n) == 0 or S == 0:
        return None
    w = int(orc.philox(seed, [gid & 0xFFFFFFFF, gid >> 32, TAG, ply])[0])
    r = (w * S) >> 32
    acc = 0
    for j, v in enumerate(n):
        acc += v
        if acc > r:
            return j
    raise AssertionError("r < S")


def played_child(orc, tree, seed, gid, ply, T):
    """(the root child self-play plays at `ply` with temperature_plies = T, whether the rule drew it): the draw
    while ply < T, else, and where the rule draws nothing, the last maximum of N; None without a child."""
    k = best_child(tree)
    if k is None or ply >= T:
        return k, False
    d = pick(orc, seed, gid, ply, children(tree)["N"])
    return (k, False) if d is None else (d, True)


def search_tree(orc, pos, sims, c_puct, seed, train_noise=0, game_id=0, ply=0):
    """(pi [2, 25], tree) of the oracle's search from scratch, root noise keyed by (seed, game_id, ply)."""
    cfg = orc.search_cfg(sims=sims, c_puct=c_puct, evaluator=orc.EVAL_HASH, train_noise=train_noise, seed=seed,
                         game_id=game_id, ply=ply)
    _, pi, nodes, _ = orc.search(cfg, pos)
    return pi, nodes


def predicted_selfplay_game(orc, game_id, sims, c_puct, R, max_plies, seed, T, deck=None, train_noise=0):
    """tree_reuse_util.predicted_selfplay_game with the temperature rule: a fresh orc.search per ply (kept + sims
    playouts, kept = kept_visits of the played child when R > 0), the rule's child while ply < T, else the last
    maximum. Returns (samples, moves, info): the game's move sequence as tuples, and info = dict(kept, fresh:
    plies whose search began on a kept / fresh tree; draws, differ: plies that drew / whose draw is not the last
    maximum; kept_other: kept subtrees of a child that is not the last maximum)."""
    s = orc.initial_state(deck if deck is not None else orc.deal_deck(seed, game_id))
    out, moves, kept = [], [], 0
    info = dict(kept=0, fresh=0, draws=0, differ=0, kept_other=0)
    res = _abi.IN_PROGRESS
    for ply in range(max_plies + 2):
        info["kept"], info["fresh"] = info["kept"] + (kept > 0), info["fresh"] + (kept == 0)
        pi, tree = search_tree(orc, s, kept + sims, c_puct, seed, train_noise, game_id, ply)
        rec = np.zeros(1, dtype=_abi.SAMPLE_DTYPE)
        rec["state"][0], rec["pi"][0] = s[0], pi.reshape(-1)
        out.append(rec)
        k, drew = played_child(orc, tree, seed, game_id, ply, T)
        if k is None:  # no legal move: pass with the mover's first card (Q6)
            mv, kept = (25, 25, 0, 2 if int(s["to_move"][0]) else 0), 0
        else:
            other = k != best_child(tree)
            info["draws"], info["differ"] = info["draws"] + drew, info["differ"] + (drew and other)
            mv = unpack(children(tree)[k]["mv"])
            kept = kept_visits(orc, tree, s, k, sims, R) if R else 0
            info["kept_other"] += bool(kept and other)
        moves.append(mv)
        s, res = stepped(orc, s, mv)
        if res in (1, 2):
            break
    out = np.concatenate(out)
    red_moved = out["state"]["to_move"] == 0  # z = reward(result, mover) (train.rs:83-85), 0 at the ply cut
    out["z"] = np.where((res == 1) == red_moved, 1.0, -1.0) if res in (1, 2) else 0.0
    return out, tuple(moves), info
