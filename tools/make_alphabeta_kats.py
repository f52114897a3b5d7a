#!/usr/bin/env python3
"""Writes tests/golden/alphabeta_kats.json from the CPU restatement of the reference's alpha-beta agent
(tests/c/alphabeta_ref.c, compiled here with gcc/cc against the oracle library, the way
tests/test_c_abi.py compiles its C). Data only: evaluation cases, roots with move and score at
max_depth 4 and 6, AlphaBeta-vs-AlphaBeta games and hand-built positions.

    python tools/make_alphabeta_kats.py            # rewrite the golden file
    python tools/make_alphabeta_kats.py --check    # compare the file with a fresh generation

tests/test_alpha_beta.py runs generate() into a temporary directory and compares (golden freshness)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))
sys.path.insert(0, str(ROOT / "tests"))
GOLDEN = ROOT / "tests" / "golden" / "alphabeta_kats.json"
NONE = 255  # move_result: Option::None (tests/c/alphabeta_ref.c ABREF_NONE)
INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1

EVAL_SEED, EVAL_N = 7101, 512
D4_SEED, D4_N = 7102, 256
D6_SEED, D6_N = 7103, 32
GAME_SEED, GAME_N, GAME_DEPTH, GAME_MAX_PLIES = 7104, 8, 4, 150

# Hand-built positions: (name, kings [red, blue], pawns [red, blue], cards R0 R1 B2 B3 N4, to_move, max_depth).
# Squares are row * 5 + col from the top left, bit 31 - square (include/onitama_az.h).
def _bb(*squares):
    b = 0
    for sq in squares:
        b |= 0x80000000 >> sq
    return b


HAND = [
    # a root without a legal move, for each colour: the mover's five pieces fill its far row and its cards
    # (Boar, Crab) only move forward or sideways, so every move leaves the board or lands on an own piece
    ("no_move_red", [_bb(0), _bb(17)], [_bb(1, 2, 3, 4), _bb(12)], [13, 4, 2, 3, 0], 0, 4),
    ("no_move_blue", [_bb(7), _bb(24)], [_bb(12), _bb(20, 21, 22, 23)], [2, 3, 13, 4, 0], 1, 4),
    # an interior node without a legal move: the same positions with the other side to move, whose quiet
    # moves all leave the opponent without a move, so the untouched INT32_MIN / INT32_MAX travels up
    ("interior_no_move_blue_root", [_bb(0), _bb(17)], [_bb(1, 2, 3, 4), _bb(12)], [13, 4, 2, 3, 0], 1, 4),
    ("interior_no_move_red_root", [_bb(7), _bb(24)], [_bb(12), _bb(20, 21, 22, 23)], [2, 3, 13, 4, 0], 0, 4),
    # mate in one, by king capture and by temple, for each colour
    ("mate_capture_red", [_bb(7), _bb(2)], [_bb(21), _bb(14)], [4, 5, 2, 3, 0], 0, 4),
    ("mate_capture_blue", [_bb(22), _bb(17)], [_bb(10), _bb(3)], [2, 3, 4, 5, 0], 1, 4),
    ("mate_temple_red", [_bb(7), _bb(14)], [_bb(21), _bb(3)], [4, 5, 2, 3, 0], 0, 4),
    ("mate_temple_blue", [_bb(10), _bb(17)], [_bb(21), _bb(3)], [2, 3, 4, 5, 0], 1, 4),
]


def build_ref(out_dir: Path):
    """tests/c/alphabeta_ref.c -> out_dir/libalphabeta_ref.so (linked to the oracle library); None without a
    C compiler."""
    import oracle_ffi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        return None
    oracle_ffi.load()  # builds oracle/build/liboaz_oracle.so when missing
    so = Path(out_dir) / "libalphabeta_ref.so"
    odir = oracle_ffi.ORACLE_SO.parent
    subprocess.run([cc, "-O2", "-std=c11", "-Wall", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(ROOT / "tests/c/alphabeta_ref.c"), f"-I{ROOT / 'oracle'}", f"-L{odir}", "-loaz_oracle",
                    f"-Wl,-rpath,{odir}", "-lm"], check=True)
    lib = C.CDLL(str(so))
    V = C.c_void_p
    lib.abref_evaluate_batch.restype, lib.abref_evaluate_batch.argtypes = None, [V, V, C.c_int, V]
    lib.abref_search.restype = C.c_int
    lib.abref_search.argtypes = [V, C.c_int, V, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.abref_play.restype = C.c_int
    lib.abref_play.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), V,
                               C.c_int]
    return lib


def ref_evaluate(lib, states: np.ndarray, move_results: np.ndarray) -> np.ndarray:
    from onitama_az import _abi
    states = np.ascontiguousarray(states, dtype=_abi.STATE_DTYPE)
    mr = np.ascontiguousarray(move_results, dtype=np.uint8)
    out = np.zeros(len(states), dtype=np.int32)
    lib.abref_evaluate_batch(_abi.ptr(states), _abi.ptr(mr), len(states), _abi.ptr(out))
    return out


def ref_search(lib, root: np.ndarray, max_depth: int):
    """(move tuple (from, to, piece, slot), score, positions, interior nodes without a legal move)."""
    from onitama_az import _abi
    root = np.ascontiguousarray(root.reshape(1), dtype=_abi.STATE_DTYPE)
    mv = np.zeros(1, dtype=_abi.MOVE_DTYPE)
    score, pos, stuck = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = lib.abref_search(_abi.ptr(root), max_depth, _abi.ptr(mv), C.byref(score), C.byref(pos), C.byref(stuck))
    assert rc == 0, rc
    return tuple(int(x) for x in mv[0]), score.value, pos.value, stuck.value


def ref_play(lib, deal_seed: int, game: int, max_depth: int, max_plies: int):
    from onitama_az import _abi
    moves = np.zeros(max_plies + 8, dtype=_abi.MOVE_DTYPE)
    res, plies = C.c_int(0), C.c_int(0)
    rc = lib.abref_play(deal_seed, game, max_depth, max_plies, C.byref(res), C.byref(plies), _abi.ptr(moves), len(moves))
    assert rc == 0, rc
    return res.value, plies.value, [[int(x) for x in m] for m in moves[: plies.value]]


def state_to_json(s) -> list:
    return [int(s["kings"][0]), int(s["kings"][1]), int(s["pawns"][0]), int(s["pawns"][1]),
            [int(c) for c in s["cards"]], int(s["to_move"])]


def states_from_json(rows) -> np.ndarray:
    from onitama_az import _abi
    a = np.zeros(len(rows), dtype=_abi.STATE_DTYPE)
    for i, (k0, k1, p0, p1, cards, tm) in enumerate(rows):
        a["kings"][i], a["pawns"][i], a["cards"][i], a["to_move"][i] = (k0, k1), (p0, p1), cards, tm
    return a


def search_roots(orc, n: int, seed: int) -> np.ndarray:
    """The first n seeded random positions that are non-terminal and have a legal move."""
    from conftest import random_positions
    pool = random_positions(orc, 2 * n + 64, seed=seed)
    keep = [s for s in pool if orc.current_state(s) == 3 and len(orc.movegen(s)) > 0]
    assert len(keep) >= n
    return np.stack(keep[:n])


def generate(lib) -> dict:
    import oracle_ffi as orc
    from conftest import random_positions
    ev_states = random_positions(orc, EVAL_N, seed=EVAL_SEED)
    ev_mr = np.array([(NONE, 0, 3, 1, 2)[i % 5] for i in range(EVAL_N)], dtype=np.uint8)
    ev = ref_evaluate(lib, ev_states, ev_mr)
    out = {
        "about": "tools/make_alphabeta_kats.py from tests/c/alphabeta_ref.c; states are [king_red, king_blue, "
                 "pawns_red, pawns_blue, cards[5], to_move], moves [from, to, piece, slot], move_result 255 = None",
        "evaluate": {"seed": EVAL_SEED, "states": [state_to_json(s) for s in ev_states],
                     "move_result": [int(x) for x in ev_mr], "value": [int(x) for x in ev]},
    }
    for key, seed, n, depth in (("depth4", D4_SEED, D4_N, 4), ("depth6", D6_SEED, D6_N, 6)):
        roots = search_roots(orc, n, seed)
        res = [ref_search(lib, r, depth) for r in roots]
        out[key] = {"seed": seed, "max_depth": depth, "states": [state_to_json(s) for s in roots],
                    "move": [list(r[0]) for r in res], "score": [r[1] for r in res],
                    "positions": [r[2] for r in res]}
    games = [ref_play(lib, GAME_SEED, g, GAME_DEPTH, GAME_MAX_PLIES) for g in range(GAME_N)]
    out["games"] = {"seed": GAME_SEED, "max_depth": GAME_DEPTH, "max_plies": GAME_MAX_PLIES,
                    "result": [g[0] for g in games], "plies": [g[1] for g in games], "moves": [g[2] for g in games]}
    hand = []
    for name, kings, pawns, cards, to_move, depth in HAND:
        s = states_from_json([[kings[0], kings[1], pawns[0], pawns[1], cards, to_move]])
        mv, score, pos, stuck = ref_search(lib, s[0], depth)
        hand.append({"name": name, "state": state_to_json(s[0]), "max_depth": depth, "move": list(mv), "score": score,
                     "legal_moves": int(len(orc.movegen(s[0]))), "interior_without_move": stuck})
    out["hand"] = hand
    return out


def dumps(d: dict) -> str:
    return json.dumps(d, separators=(",", ":")) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_ref(Path(tmp))
        if lib is None:
            print("no C compiler: skipped")
            return 0
        text = dumps(generate(lib))
    if args.check:
        ok = GOLDEN.read_text() == text
        print("golden is fresh" if ok else "golden DIFFERS from a fresh generation")
        return 0 if ok else 1
    GOLDEN.write_text(text)
    print(f"wrote {GOLDEN} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
