"""Shared by the arena tests: evaluator.rs:355-399 restated one game after the other on the host, for a
HASH-evaluator AlphaZero agent (the oracle's search) against the Random agent (oaz_random_agent_move), stepped
by the oracle's make_move and the pass rule. Needs no GPU."""
import numpy as np

from onitama_az import _abi

C_PUCT = 2.0 ** 0.5


def sequential_hash_vs_random(orc, lib, game_amnt, max_plies, deal_seed, random_seed, sims, deck=None, starts=None):
    """Returns (results, plies, passes, quirk_games): per game the last MoveResult and the moves made; the passes
    over all games; and the games in which Random moved as Blue before the game's last ply (its used_card_idx
    0 / 1 then rotated one of Red's cards: the quirk shaped the rest of the game)."""
    results, plies, passes, quirk_games = [], [], 0, 0
    cfg = orc.search_cfg(sims=sims, c_puct=C_PUCT, evaluator=orc.EVAL_HASH, train_noise=0)
    for k in range(game_amnt):
        if starts is not None:  # (oaz_arena_config.start)
            s = np.ascontiguousarray(starts[k:k + 1]).copy()
        else:
            s = orc.initial_state(deck if deck is not None else orc.deal_deck(deal_seed, k))
        agent_colour = k % 2  # the agent is Red in even games
        progress, budget, n, blue_random_plies = _abi.IN_PROGRESS, max_plies, 0, []
        while progress not in (_abi.RED_WIN, _abi.BLUE_WIN):
            mover = int(s["to_move"][0])
            if mover == agent_colour:
                mv = orc.search(cfg, s[0], tree=False)[0]
                mv = tuple(int(mv[f]) for f in ("from_", "to", "piece", "slot"))
            else:
                out = np.zeros(1, dtype=_abi.MOVE_DTYPE)
                assert lib.oaz_random_agent_move(random_seed, k, n, _abi.ptr(np.ascontiguousarray(s)), _abi.ptr(out)) == 0
                mv = tuple(int(out[0][f]) for f in ("from_", "to", "piece", "slot"))
                if mover == 1:
                    blue_random_plies.append(n)
            if mv[0] >= 25:  # pass (state.rs:139-142)
                c = s["cards"][0].copy()
                c[mv[3]], c[4] = c[4], c[mv[3]]
                s["cards"][0] = c
                progress = _abi.IN_PROGRESS
                passes += 1
            else:
                progress = orc.make_move(s, mv, mover)
            s["to_move"][0] ^= 1
            n += 1
            if budget < 0:
                break
            budget -= 1
        results.append(int(progress))
        plies.append(n)
        quirk_games += any(p < n - 1 for p in blue_random_plies)
    return results, plies, passes, quirk_games
