"""Leaf-parallel search (oaz_config.leaf_batch), the parts that need no GPU: the Python statement of the rule
(tests/leaf_batch_ref.py) against the sequential restatement (tests/pyref.py) and its own invariants, and the
config layout."""
import ctypes as C

import numpy as np
import pytest

import leaf_batch_ref as lbr
import pyref
from leaf_batch_util import sparse_endgame, start_root
from onitama_az import _abi


def _same_arena(a, b):
    if len(a) != len(b):
        return False
    return all((x.parent, x.mov, x.color, x.prob, x.children, x.visits, x.reward, x.terminal, x.expanded) ==
               (y.parent, y.mov, y.color, y.prob, y.children, y.visits, y.reward, y.terminal, y.expanded)
               for x, y in zip(a, b))


def test_leaf_batch_one_is_the_sequential_search(orc):
    """L = 1 reproduces pyref.search node for node (start position, 200 playouts, c = 5): W - 0.0 == W, one
    leaf per round, never a collision."""
    root = lbr.state_of(start_root(orc, 0))
    mv, pi, arena, (rounds, discarded) = lbr.search(root, 200, 5.0, 1)
    ref_mv, ref_pi, ref_arena = pyref.search(root, 200, 5.0)
    assert _same_arena(arena, ref_arena)
    assert all(x.winrate == (x.reward / x.visits if x.visits else 0.0) for x in ref_arena)
    assert mv == ref_mv and pi == ref_pi and (rounds, discarded) == (200, 0)


@pytest.fixture(scope="module")
def sequential_100(orc):
    return lbr.search(lbr.state_of(start_root(orc, 0)), 100, 5.0, 1)[2]


@pytest.mark.parametrize("L", [2, 7, 16])
def test_root_visits_and_in_flight_counts(orc, L, sequential_100):
    """Root visits = sims and every v is 0 at the end, for sims in {1, 2, L + 1, 100}; the first round has one
    leaf (the root is unexpanded); at 100 playouts the tree differs from the L = 1 tree (the rule uses L)."""
    root = lbr.state_of(start_root(orc, 0))
    for sims in (1, 2, L + 1, 100):
        mv, pi, arena, (rounds, discarded) = lbr.search(root, sims, 5.0, L)
        assert arena[0].visits == sims and all(n.v == 0 for n in arena)
        assert sum(arena[c].visits for c in arena[0].children) == sims - 1
        assert 1 + (sims - 1 + L - 1) // L <= rounds <= sims  # round 1: one leaf; later rounds: 1 .. L leaves
        if sims >= 100:
            assert rounds < sims and not _same_arena(arena, sequential_100)


def test_won_leaves_repeat_within_a_round():
    """The sparse endgame: Red's winning capture is terminal-flagged on the first walk through it, and the walks of
    one round end on it again and again without a collision (a collision needs an unexpanded, unflagged leaf)."""
    root = lbr.state_of(sparse_endgame(0))
    mv, pi, arena, (rounds, discarded) = lbr.search(root, 60, 5.0, 16)
    won = [c for c in arena[0].children if arena[c].terminal]
    assert won and max(arena[c].visits for c in won) > rounds  # more visits than rounds: repeats inside a round
    assert arena[0].visits == 60 and all(n.v == 0 for n in arena)


def test_config_layout_leaf_batch_took_a_pad_byte(lib):
    assert _abi.oaz_config.leaf_batch.offset == 70 and _abi.oaz_config.leaf_batch.size == 1
    assert _abi.oaz_config.temperature_plies.offset == 69 and _abi.oaz_config.seed.offset == 72
    assert C.sizeof(_abi.oaz_config) == 120 and _abi.oaz_config.reuse_visits.offset == 116
    assert lib.oaz_abi_version() == _abi.ABI_VERSION == 5
    assert _abi.default_config().leaf_batch == 0


def test_leaf_batch_above_16_is_rejected_at_creation(lib):
    """Checked before a device is touched, like every other field of the config."""
    cfg = _abi.default_config()
    cfg.leaf_batch = 17
    assert not lib.oaz_create(C.byref(cfg), 0)
    assert b"leaf_batch" in lib.oaz_last_error()


def test_leaf_batch_stats_null_arguments(lib):
    out = (C.c_uint64 * 3)()
    assert lib.oaz_search_leaf_batch_stats(None, C.byref(out)) == _abi.ERR_ARG


def test_agent_config_carries_leaf_batch():
    from onitama_az.mcts import AlphaZeroMctsConfig
    assert AlphaZeroMctsConfig().leaf_batch == 0 and AlphaZeroMctsConfig(leaf_batch=8).leaf_batch == 8
