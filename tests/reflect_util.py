"""Shared helpers of the reflection tests (tests/test_reflect.py, tests/test_gpu_reflect.py): the left-right
reflection restated in numpy, independently of the C code (loops over squares, no bit tricks), and seeded
random-play records from the oracle's rules.

The transformation (include/onitama_az.h, "left-right reflection"): square i -> R(i) = 5 (i / 5) + 4 - i % 5 (25,
the pass move's square, fixed); the bit of square i, 1 << (31 - i), moves to the bit of R(i); card k -> CARDS[k];
a state's four bitboards and five cards go through these, to_move and pad stay; a move's from and to go through
R; a record's pi'[k][R(t)] = pi[k][t], z stays.
"""
import random
from types import SimpleNamespace

import numpy as np

from onitama_az import _abi

# 0 Tiger 1 Dragon 2 Frog 3 Rabbit 4 Crab 5 Elephant 6 Goose 7 Rooster 8 Monkey 9 Mantis 10 Crane 11 Horse 12 Ox
# 13 Boar 14 Eel 15 Cobra: Frog<->Rabbit, Goose<->Rooster, Horse<->Ox, Eel<->Cobra
CARDS = [0, 1, 3, 2, 4, 5, 7, 6, 8, 9, 10, 12, 11, 13, 15, 14]


def R(i):
    if i == 25:
        return 25
    row, col = divmod(i, 5)
    return 5 * row + (4 - col)


def reflect_board(b):
    out = 0
    for i in range(25):
        if (int(b) >> (31 - i)) & 1:
            out |= 1 << (31 - R(i))
    return out


def reflect_boards(b):
    """reflect_board over a uint32 array (a loop over the squares, every element at once)."""
    b = np.asarray(b, dtype=np.uint32)
    out = np.zeros_like(b)
    for i in range(25):
        out |= ((b >> np.uint32(31 - i)) & np.uint32(1)) << np.uint32(31 - R(i))
    return out


def reflect_states(states):
    out = states.copy()
    for n in range(len(states)):
        for c in range(2):
            out["kings"][n][c] = reflect_board(states["kings"][n][c])
            out["pawns"][n][c] = reflect_board(states["pawns"][n][c])
        for k in range(5):
            out["cards"][n][k] = CARDS[int(states["cards"][n][k])]
    return out


def reflect_moves(moves):
    out = moves.copy()
    flat_in, flat_out = moves.reshape(-1), out.reshape(-1)
    for n in range(flat_in.size):
        flat_out["from_"][n] = R(int(flat_in["from_"][n]))
        flat_out["to"][n] = R(int(flat_in["to"][n]))
    return out


def reflect_pi(pi):
    """pi [n, 50] keyed [hand slot][to]: out[k][R(t)] = pi[k][t]."""
    out = np.zeros_like(pi)
    for k in range(2):
        for t in range(25):
            out[:, k * 25 + R(t)] = pi[:, k * 25 + t]
    return out


def reflect_samples(samples):
    out = samples.copy()
    out["state"] = reflect_states(np.ascontiguousarray(samples["state"]))
    out["pi"] = reflect_pi(samples["pi"])
    return out


def reflect_planes(planes):
    """create_tensor_from_state planes [n, 21, 5, 5] of the reflected states, from those of the states: planes 0-3
    (the pieces) flipped along the column axis, card plane 4 + k moved to 4 + CARDS[k], plane 20 (the colour) kept."""
    out = np.zeros_like(planes)
    for p in range(4):
        for col in range(5):
            out[:, p, :, 4 - col] = planes[:, p, :, col]
    for k in range(16):
        out[:, 4 + CARDS[k]] = planes[:, 4 + k]
    out[:, 20] = planes[:, 20]
    return out


def card_map_from_attack(att):
    """The card map derived from ATTACK_MAPS [2][16][25]: for every card the cards k2 with
    reflect(att[c][k][f]) == att[c][k2][R(f)] for both colours and all squares (a list per card)."""
    out = []
    for k in range(16):
        out.append([k2 for k2 in range(16) if all(
            reflect_board(att[c][k][f]) == int(att[c][k2][R(f)]) for c in range(2) for f in range(25))])
    return out


def move_set(moves):
    return {(int(m["from_"]), int(m["to"]), int(m["piece"]), int(m["slot"])) for m in moves}


_PLAY = {}


def random_play(orc, n, seed):
    """At least n records of seeded random play with the oracle's rules, whole games with random decks: states[i]
    (to_move = the mover), the move played moves[i], its MoveResult results[i] and the position after it after[i]
    (to_move switched). Computed once per (n, seed) and shared; do not change the arrays."""
    if (n, seed) in _PLAY:
        return _PLAY[(n, seed)]
    rng = random.Random(seed)
    states, moves, results, after = [], [], [], []
    game = 0
    while len(states) < n:
        s = orc.initial_state(orc.deal_deck(seed, game))
        game += 1
        for _ in range(150):
            legal = orc.movegen(s)
            if len(legal) == 0:
                break
            m = legal[rng.randrange(len(legal))]
            states.append(s.copy())
            moves.append(m.copy())
            r = orc.make_move(s, tuple(int(m[k]) for k in ("from_", "to", "piece", "slot")), int(s["to_move"][0]))
            s["to_move"][0] ^= 1
            results.append(r)
            after.append(s.copy())
            if r in (_abi.RED_WIN, _abi.BLUE_WIN):
                break
    out = SimpleNamespace(states=np.concatenate(states), moves=np.array(moves, dtype=_abi.MOVE_DTYPE),
                          results=np.array(results, dtype=np.uint8), after=np.concatenate(after))
    for a in (out.states, out.moves, out.results, out.after):
        a.setflags(write=False)
    _PLAY[(n, seed)] = out
    return out


def assert_both_colours_capture_and_win(play):
    """The records hold captures and wins of both colours (so the equivariance of those paths is checked)."""
    mover = play.states["to_move"]
    for colour in (0, 1):
        assert np.any((play.results == _abi.CAPTURE) & (mover == colour)), colour
    assert np.any(play.results == _abi.RED_WIN) and np.any(play.results == _abi.BLUE_WIN)


def random_samples(play, n, seed):
    """n records on the first n random-play positions with random pi (sparse, normalised) and z in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    samples = np.zeros(n, dtype=_abi.SAMPLE_DTYPE)
    samples["state"] = play.states[:n]
    pi = rng.random((n, 50)) * (rng.random((n, 50)) < 0.3)
    pi[:, 0] += 1e-3  # never an all-zero row
    samples["pi"] = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    samples["z"] = rng.integers(-1, 2, n).astype(np.float32)
    return samples
