"""onitama_az.parameter_check: alphazero-training/src/bin/mcts_parameter_check.rs as one lock-step fight.

CPU: the pairings' order, the printed lines, the fold of a pairing's results, and the host restatement of a
pairing (`restate_pairing`: the oracle's rules and orc.pure_mcts, one game after the other), which is the checker
of the GPU test: the sweep's games must equal it game for game, and pairing after pairing must equal lock step.
"""
import numpy as np
import pytest

from onitama_az import _abi
from onitama_az.parameter_check import (C_VALUES, N_VALUES, ParameterCheck, PairingResult, fold_results, format_line,
                                        pairings)
from onitama_az.pure_mcts import default_config


def restate_pairing(orc, kind, first, second, p, game_amnt, max_playouts, max_plies, seed, min_node_visits=1,
                    exploration_c=1.0):
    """mcts_parameter_check.rs:8-47 for pairing number p, one game after the other: game j is the sweep's game
    q = p * game_amnt + j (dealt deal_deck(seed, q)), the first-named value plays Red in even games, and the
    search at ply t draws from stream (t << 20) + q. Returns (results, plies) per game."""
    results, plies = [], []
    for j in range(game_amnt):
        q = p * game_amnt + j
        s = orc.initial_state(orc.deal_deck(seed, q))
        progress, budget, t = _abi.IN_PROGRESS, max_plies, 0
        while progress not in (_abi.RED_WIN, _abi.BLUE_WIN):
            mover = int(s["to_move"][0])
            value = first if (mover == 0) == (j % 2 == 0) else second
            cfg = default_config()
            cfg.max_playouts, cfg.seed = max_playouts, seed
            cfg.min_node_visits = int(value) if kind == "n" else min_node_visits
            cfg.exploration_c = float(value) if kind == "c" else exploration_c
            mv = orc.pure_mcts(cfg, (t << 20) + q, s[0])[0]
            mv = tuple(int(mv[f]) for f in ("from_", "to", "piece", "slot"))
            if mv[0] >= 25:  # pass (state.rs:139-142)
                c = s["cards"][0].copy()
                c[mv[3]], c[4] = c[4], c[mv[3]]
                s["cards"][0] = c
                progress = _abi.IN_PROGRESS
            else:
                progress = orc.make_move(s, mv, mover)
            s["to_move"][0] ^= 1
            t += 1
            if budget < 0:
                break
            budget -= 1
        results.append(int(progress))
        plies.append(t)
    return results, plies


def test_values_and_pairings_in_the_reference_order():
    assert C_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0) and N_VALUES == (0, 1, 2, 3, 4, 5, 6, 7, 8)
    pc, pn = pairings(C_VALUES), pairings(N_VALUES)
    assert len(pc) == 21 and len(pn) == 36
    assert pc[:7] == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2)] and pc[-1] == (5, 6)
    assert pn == [(i, k) for i in range(9) for k in range(i + 1, 9)]
    assert pairings((1.0,)) == [] and pairings(()) == []


def test_printed_lines():
    assert format_line("c", 0.0, 0.5, 0.37) == "MCTS with c = 0.00 vs MCTS with c = 0.50 -> winrate: 0.37"
    assert format_line("n", 0, 3, 0.5) == "MCTS with n = 0 vs MCTS with n = 3 -> winrate: 0.50"
    assert format_line("c", 2.5, 3.0, 1.0).endswith("winrate: 1.00")


def test_fold_alternates_colours_and_counts_a_cut_game_as_no_win():
    R, B, CUT = _abi.RED_WIN, _abi.BLUE_WIN, _abi.IN_PROGRESS
    # game 0 (first is Red): Red wins -> win; game 1 (first is Blue): Red wins -> loss; game 2: cut; game 3
    # (first is Blue): Blue wins -> win; game 4 (first is Red): Blue wins -> loss; game 5: a capture is no win
    assert fold_results([R, R, CUT, B, B, _abi.CAPTURE]) == (2, 2)
    assert fold_results([]) == (0, 0)
    assert fold_results([B, R]) == (0, 0) and fold_results([R, B]) == (2, 0)


def test_configuration_checks():
    with pytest.raises(ValueError):
        ParameterCheck("x", (0, 1))
    with pytest.raises(ValueError):
        ParameterCheck("n", N_VALUES, game_amnt=(1 << 20) // 36 + 1)
    pc = ParameterCheck("c", C_VALUES)
    assert (pc.game_amnt, pc.max_playouts, pc.search_time, pc.min_node_visits, pc.max_plies) == (100, 1600, 0.4, 1, 150)
    assert ParameterCheck("n", N_VALUES).exploration_c == 1.0 and not pc.enforce_search_time


def test_host_restatement_is_deterministic(orc):
    a = restate_pairing(orc, "c", 0.0, 2.5, 1, 3, 24, 20, seed=11)
    b = restate_pairing(orc, "c", 0.0, 2.5, 1, 3, 24, 20, seed=11)
    assert a == b and len(a[0]) == 3
    assert all(1 <= n <= 22 for n in a[1])
    assert all((r in (_abi.RED_WIN, _abi.BLUE_WIN)) or n == 22 for r, n in zip(*a))


SWEEP = dict(game_amnt=4, max_playouts=48, max_plies=30, verbose=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,values", [("c", (0.0, 1.0, 2.5)), ("n", (0, 1, 5))])
def test_gpu_sweep_equals_the_host_restatement(orc, kind, values):
    pc = ParameterCheck(kind, values, **SWEEP)
    got = pc.play()
    assert pc.launches == max(max(r.plies) for r in got) and len(got) == 3
    cut = won = 0
    for p, ((i, k), r) in enumerate(zip(pairings(values), got)):
        assert isinstance(r, PairingResult) and (r.first, r.second) == (values[i], values[k])
        results, plies = restate_pairing(orc, kind, values[i], values[k], p, 4, 48, 30, seed=pc.seed)
        assert (r.results, r.plies) == (results, plies), (kind, p)
        assert (r.wins, r.cut) == fold_results(results) and r.winrate == r.wins / 4
        cut += r.cut
        won += len(results) - r.cut
    assert cut >= 1 and won >= 1  # both ends of a game are exercised
    again = ParameterCheck(kind, values, **SWEEP)
    seq = again.play(sequential=True)
    assert seq == got and again.launches == sum(max(r.plies) for r in got)
