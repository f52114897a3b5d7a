#!/usr/bin/env python3
"""Writes tests/golden/alphabeta_deep_kats.json: the CPU restatement of the reference's alpha-beta agent
(tests/c/alphabeta_ref.c, through tools/make_alphabeta_kats.py) at the depths only the split search
(oaz_alphabeta_generate_move) answers. Data only:

  - depth7: 16 seeded roots with move, score and positions at max_depth 7;
  - depth8: 4 seeded roots at max_depth 8 (the tournament's depth; each under a second on one CPU thread);
  - hand: the 8 hand-built positions of make_alphabeta_kats.HAND at every max_depth 3..8 (roots, interior nodes
    and frontier items without a legal move; mates in one, so winning moves inside the expanded levels);
  - games: two AlphaBeta(7)-vs-Random games under fight's loop (evaluator.rs:373-389), AlphaBeta playing Red
    in game 0 and Blue in game 1, the Random side's moves from the host-only oaz_random_agent_move keyed by
    (seed, game, ply), so the whole game is reproducible without a GPU.

    python tools/make_alphabeta_deep_kats.py            # rewrite the golden file
    python tools/make_alphabeta_deep_kats.py --check    # compare the file with a fresh generation

tests/test_alpha_beta_deep.py runs generate() and compares (golden freshness)."""
from __future__ import annotations

import argparse
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import make_alphabeta_kats as base  # noqa: E402  (puts the package and tests/ on sys.path)

GOLDEN = ROOT / "tests" / "golden" / "alphabeta_deep_kats.json"
D7_SEED, D7_N = 7105, 16
D8_SEED, D8_N = 7106, 4
HAND_DEPTHS = (3, 4, 5, 6, 7, 8)
GAME_SEED, GAME_N, GAME_DEPTH, GAME_MAX_PLIES = 7107, 2, 7, 30


def play_vs_random(lib, orc, seed: int, game: int, max_depth: int, max_plies: int):
    """(last MoveResult, plies, moves): game `game` of a fight of AlphaBeta(max_depth) against the Random agent
    keyed by `seed`, dealt oaz_deal_deck(seed, game); AlphaBeta is Red in even games."""
    from onitama_az import _abi
    oaz = _abi.load()
    s = orc.initial_state(orc.deal_deck(seed, game))
    ab_red = game % 2 == 0
    progress, budget, moves = _abi.IN_PROGRESS, max_plies, []
    while progress not in (_abi.RED_WIN, _abi.BLUE_WIN):
        color = int(s["to_move"][0])
        if (color == 0) == ab_red:
            mv = base.ref_search(lib, s[0], max_depth)[0]
        else:
            out = np.zeros(1, dtype=_abi.MOVE_DTYPE)
            _abi.check(oaz.oaz_random_agent_move(seed, game, len(moves), _abi.ptr(s), _abi.ptr(out)))
            mv = tuple(int(x) for x in out[0])
        moves.append(list(mv))
        if mv[0] >= 25:  # a pass (State::pass, state.rs:139-142): the named card goes round
            cards = s["cards"][0].copy()
            cards[mv[3]], cards[4] = cards[4], cards[mv[3]]
            s["cards"][0] = cards
            progress = _abi.IN_PROGRESS
        else:
            progress = orc.make_move(s, mv, color)
        s["to_move"][0] ^= 1
        if budget < 0:
            break
        budget -= 1
    return int(progress), len(moves), moves


def generate(lib) -> dict:
    import oracle_ffi as orc
    out = {"about": "tools/make_alphabeta_deep_kats.py from tests/c/alphabeta_ref.c; states, moves and results as in "
                    "alphabeta_kats.json"}
    for key, seed, n, depth in (("depth7", D7_SEED, D7_N, 7), ("depth8", D8_SEED, D8_N, 8)):
        roots = base.search_roots(orc, n, seed)
        res = [base.ref_search(lib, r, depth) for r in roots]
        out[key] = {"seed": seed, "max_depth": depth, "states": [base.state_to_json(s) for s in roots],
                    "move": [list(r[0]) for r in res], "score": [r[1] for r in res], "positions": [r[2] for r in res]}
    hand = []
    for name, kings, pawns, cards, to_move, _ in base.HAND:
        s = base.states_from_json([[kings[0], kings[1], pawns[0], pawns[1], cards, to_move]])
        res = {d: base.ref_search(lib, s[0], d) for d in HAND_DEPTHS}
        hand.append({"name": name, "state": base.state_to_json(s[0]), "max_depth": list(HAND_DEPTHS),
                     "move": [list(res[d][0]) for d in HAND_DEPTHS], "score": [res[d][1] for d in HAND_DEPTHS],
                     "interior_without_move": [res[d][3] for d in HAND_DEPTHS]})
    out["hand"] = hand
    games = [play_vs_random(lib, orc, GAME_SEED, g, GAME_DEPTH, GAME_MAX_PLIES) for g in range(GAME_N)]
    out["games"] = {"seed": GAME_SEED, "max_depth": GAME_DEPTH, "max_plies": GAME_MAX_PLIES,
                    "result": [g[0] for g in games], "plies": [g[1] for g in games], "moves": [g[2] for g in games]}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        lib = base.build_ref(Path(tmp))
        if lib is None:
            print("no C compiler: skipped")
            return 0
        text = base.dumps(generate(lib))
    if args.check:
        ok = GOLDEN.read_text() == text
        print("golden is fresh" if ok else "golden DIFFERS from a fresh generation")
        return 0 if ok else 1
    GOLDEN.write_text(text)
    print(f"wrote {GOLDEN} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
