"""GPU: playout cap randomization (oaz_selfplay_set_playout_cap) against the unchanged oracle. Whole capped self-play
games (three fast budgets, fixed and dealt decks, short and long games, root noise, temperature, two ranks) equal
the games predicted from orc.search alone (tests/playout_cap_util.py); one ply's trees equal orc.search at the ply's
budget with the games in two and four parts; the network path's trees equal a cap-off engine's searches at the two
budgets bit for bit. Every condition on the cases themselves (plies of both kinds, games that differ from the cap-off
games, a game without a record) is checked on the oracle's prediction. HASH evaluator and blocks = 0 unless said."""
import functools

import numpy as np
import pytest

import oracle_ffi
import playout_cap_util as pcu
from onitama_az import _abi
from onitama_az.engine import Engine
from tree_reuse_util import assert_trees_equal, sorted_rows

pytestmark = pytest.mark.gpu

HASH = dict(evaluator=_abi.EVAL_HASH, blocks=0)
DECK = [0, 1, 2, 3, 4]
SEED = 4242
SIMS, SHARE, GAMES, SLOTS = 24, 16384, 24, 8


@functools.lru_cache(maxsize=None)
def _predicted(fixed, max_plies, n, P, train_noise=0, T=0, seed=SEED, sims=SIMS):
    """The 24 games from orc.search alone: (records in game order, move sequences, summed info, records per game)."""
    recs, seqs, per_game, info = [], [], [], {}
    for gid in range(GAMES):
        s, mv, i = pcu.predicted_selfplay_game(oracle_ffi, gid, sims, n, P, 5.0, max_plies, seed, T=T,
                                               deck=np.array(DECK, np.uint8) if fixed else None, train_noise=train_noise)
        recs.append(s)
        seqs.append(mv)
        per_game.append(len(s))
        info = {k: info.get(k, 0) + v for k, v in i.items()}
    return np.concatenate(recs), tuple(seqs), info, tuple(per_game)


def _selfplay(fixed, max_plies, cap, train_noise=0, T=0, slots=SLOTS, rank=0, world=1, seed=SEED, sims=SIMS):
    """(records, stats, playout_cap_stats) of the 24 games; cap = (n, P) or None."""
    kw = dict(playout_cap=cap) if cap else {}
    with Engine(games=slots, sims=sims, c_puct=5.0, max_plies=max_plies, seed=seed, fixed_deck=int(fixed), deck=DECK,
                temperature_plies=T, train_noise=train_noise, rank=rank, world=world, **HASH, **kw) as e:
        got, st = e.selfplay_run(GAMES, cap=GAMES * (max_plies + 2))
        return got, st, e.playout_cap_stats()


def _check_against_prediction(fixed, max_plies, n, train_noise=0, T=0, seed=SEED):
    ref, seqs, info, per_game = _predicted(fixed, max_plies, n, SHARE, train_noise, T, seed)
    _, seqs0, _, _ = _predicted(fixed, max_plies, n, 65536, train_noise, T, seed)  # every ply full: the cap-off games
    print(f"predicted: {info['full']} full, {info['fast']} fast plies, {len(ref)} records, "
          f"{sum(a != b for a, b in zip(seqs, seqs0))} games differ from the cap-off ones, "
          f"{sum(k == 0 for k in per_game)} games without a record")
    # (the oracle's alone) plies of both kinds, and at least half of the games differ from the games without a cap
    assert info["full"] >= 60 and info["fast"] >= 190
    assert sum(a != b for a, b in zip(seqs, seqs0)) >= 12
    if max_plies == 10:
        assert sum(k == 0 for k in per_game) >= 1  # a game without a full ply: no record, still finished
    assert len(ref) == info["full"]
    got, st, cs = _selfplay(fixed, max_plies, (n, SHARE), train_noise, T, seed=seed)
    assert st.games_finished == GAMES
    assert cs == (info["full"], info["fast"])
    assert st.moves == info["full"] + info["fast"] == sum(len(s) for s in seqs)
    assert st.search.sims == info["full"] * SIMS + info["fast"] * n
    assert len(got) == len(ref) and st.samples_dropped == 0
    assert np.array_equal(sorted_rows(got), sorted_rows(ref))


@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "dealt"])
@pytest.mark.parametrize("max_plies", [10, 150])
@pytest.mark.parametrize("n", [1, 6, 23])
def test_c1_whole_games_equal_the_prediction(orc, n, max_plies, fixed):
    """24 games on 8 slots, sims 24, P = 1/4: the records (z included) as sorted byte rows and every counter."""
    _check_against_prediction(fixed, max_plies, n)


def test_c1_whole_games_with_root_noise(orc):
    _check_against_prediction(True, 150, 6, train_noise=1)


def test_c1_whole_games_with_temperature(orc):
    _check_against_prediction(True, 150, 6, T=8)


def test_c2_every_ply_full_equals_the_cap_off_engine(orc):
    """P = 65536: the cap-off engine's records byte for byte (the capped ply ran the per-step kernels with leaf
    compaction, the cap-off one a one-launch search), and no fast ply."""
    off, st0, cs0 = _selfplay(True, 150, None)
    got, st, cs = _selfplay(True, 150, (6, 65536))
    assert cs0 == (0, 0) and st0.games_finished == GAMES and len(off) > 0
    assert got.tobytes() == off.tobytes()
    assert cs == (st0.moves, 0) and st.moves == st0.moves and st.games_finished == GAMES
    assert st.search.sims == st0.search.sims == st0.moves * SIMS
    ref = _predicted(True, 150, 6, 65536)[0]
    assert np.array_equal(sorted_rows(got), sorted_rows(ref))


def test_c2_no_ply_full_gives_no_record(orc):
    _, seqs, info, per_game = _predicted(True, 150, 6, 0)
    assert info["full"] == 0 and sum(per_game) == 0
    got, st, cs = _selfplay(True, 150, (6, 0))
    assert len(got) == 0 and st.samples_ready == 0
    assert st.games_finished == GAMES
    assert st.moves == sum(len(s) for s in seqs) == info["fast"]
    assert cs == (0, info["fast"]) and st.search.sims == info["fast"] * 6


@pytest.mark.parametrize("train_noise", [0, 1], ids=["plain", "noise"])
@pytest.mark.parametrize("parts", [2, 4])
def test_c3_parts_and_unaligned_compaction(orc, parts, train_noise):
    """70 games in 2 parts (35 + 35: the second part's need bytes and masks start unaligned) and in 4 (18, 18, 18,
    16), one ply from a reset: every slot's tree has `sims` or `n` root visits by the rule and equals orc.search at
    that budget node for node. With root noise the chunk boundary (16) lies inside phase two."""
    G, n = 70, 6
    budgets = [pcu.budget(orc, SEED, g, 0, SIMS, n, SHARE) for g in range(G)]
    assert 8 <= budgets.count(SIMS) <= 40 and budgets.count(SIMS) + budgets.count(n) == G
    with Engine(games=G, sims=SIMS, c_puct=5.0, seed=SEED, train_noise=train_noise, parts=parts,
                playout_cap=(n, SHARE), **HASH) as e:
        e.selfplay_reset()
        e.selfplay_step(1)
        assert e.kernel_times().parts == parts
        trees = [e.tree(g) for g in range(G)]
        assert e.playout_cap_stats() == (budgets.count(SIMS), budgets.count(n))
        assert e.selfplay_stats().search.sims == sum(budgets)
    for g in range(G):
        assert int(trees[g][0]["N"]) == budgets[g], g
        pos = orc.initial_state(orc.deal_deck(SEED, g))
        cfg = orc.search_cfg(sims=budgets[g], c_puct=5.0, evaluator=orc.EVAL_HASH, train_noise=train_noise, seed=SEED,
                             game_id=g, ply=0)
        assert_trees_equal(trees[g], orc.search(cfg, pos)[2])


def test_c4_two_ranks(orc):
    """Two ranks of 12 games each hold together the records of one engine playing the 24: the rule's key is the
    global game id."""
    whole, st, cs = _selfplay(True, 150, (6, SHARE))
    halves = [_selfplay(True, 150, (6, SHARE), slots=4, rank=r, world=2) for r in range(2)]
    assert [h[1].games_finished for h in halves] == [12, 12]
    both = np.concatenate([h[0] for h in halves])
    assert np.array_equal(sorted_rows(both), sorted_rows(whole))
    assert np.array_equal(sorted_rows(whole), sorted_rows(_predicted(True, 150, 6, SHARE)[0]))
    assert tuple(sum(h[2][k] for h in halves) for k in range(2)) == cs
    assert cs[0] > 0 and cs[1] > 0 and min(len(h[0]) for h in halves) > 0


def test_c5_network_path(orc):
    """The fp16x3 network, 3 blocks, the engines' random-init weights, 64 games, sims 16, n 4, no noise. After one
    ply from a reset, 16 trees equal those of a cap-off engine with the same weights searching the same start
    positions with 16 or 4 playouts, bit for bit; no tile left the fp16 range."""
    G, sims, n = 64, 16, 4
    nn = dict(evaluator=_abi.EVAL_NN, blocks=3, precision=_abi.FP32_SPLIT16, c_puct=5.0, seed=SEED, train_noise=0)
    budgets = [pcu.budget(orc, SEED, g, 0, sims, n, SHARE) for g in range(G)]
    full = [g for g in range(G) if budgets[g] == sims]
    fast = [g for g in range(G) if budgets[g] == n]
    assert len(full) >= 8 and len(fast) >= 8
    sample = full[:8] + fast[:8]
    roots = np.concatenate([orc.initial_state(orc.deal_deck(SEED, g)) for g in range(G)])
    with Engine(games=G, sims=sims, playout_cap=(n, SHARE), **nn) as e:
        e.selfplay_reset()
        e.selfplay_step(1)
        got = {g: e.tree(g) for g in sample}
        roots_n = {g: int(e.tree(g)[0]["N"]) for g in range(G)}
        assert e.nn_fallbacks() == 0
        assert e.playout_cap_stats() == (len(full), len(fast))
    assert [roots_n[g] for g in range(G)] == budgets
    with Engine(games=G, sims=sims, **nn) as e:
        for b, games in ((sims, full[:8]), (n, fast[:8])):
            e.set_search_params(b, 5.0, False)
            e.search(roots)
            for g in games:
                ref = e.tree(g)
                assert int(ref[0]["N"]) == b
                assert_trees_equal(got[g], ref)
                for f in ("W", "P"):  # bit for bit, not only equal as numbers
                    assert got[g][f].tobytes() == ref[f].tobytes(), (g, b, f)
        assert e.nn_fallbacks() == 0


@pytest.mark.parametrize("kw", [dict(reuse_visits=96), dict(leaf_batch=4), dict(search_time_ns=10 ** 9)],
                         ids=["reuse_visits", "leaf_batch", "search_time"])
def test_c6_refused_engines(kw):
    with Engine(games=8, sims=SIMS, c_puct=5.0, seed=SEED, train_noise=0, **HASH, **kw) as e:
        assert e._lib.oaz_selfplay_set_playout_cap(e.handle, 6, SHARE) == _abi.ERR_STATE
        assert e.playout_cap_stats() == (0, 0)
        assert e._lib.oaz_selfplay_set_playout_cap(e.handle, -1, SHARE) == _abi.ERR_ARG
        assert e._lib.oaz_selfplay_set_playout_cap(e.handle, 6, 65537) == _abi.ERR_ARG
    with pytest.raises(_abi.OazError):
        Engine(games=8, sims=SIMS, playout_cap=(6, SHARE), **HASH, **kw)


def test_c6_refused_steps_and_the_engine_afterwards(orc):
    roots = np.concatenate([orc.initial_state(np.array(DECK, np.uint8))] * 8)
    common = dict(games=8, sims=SIMS, c_puct=5.0, seed=SEED, train_noise=0, fixed_deck=1, deck=DECK, max_plies=150, **HASH)
    with Engine(**common) as plain:
        want = plain.search(roots)
        want_tree = plain.tree(3)
        plain.selfplay_reset()
        plain.selfplay_step(3)
        want_plies = plain.selfplay_stats().moves
    with Engine(**common) as e:
        e.set_playout_cap(SIMS, SHARE)  # n >= sims: the step refuses
        assert e._lib.oaz_selfplay_step(e.handle, 1) == _abi.ERR_STATE
        e.set_playout_cap(SIMS + 5, SHARE)
        assert e._lib.oaz_selfplay_step(e.handle, 1) == _abi.ERR_STATE
        e.set_playout_cap(6, SHARE)
        e.set_search_params(6, 5.0, False)  # sims lowered to n afterwards
        assert e._lib.oaz_selfplay_step(e.handle, 1) == _abi.ERR_STATE
        e.set_search_params(SIMS, 5.0, False)
        e.set_search_time(1.0)  # a budget set since
        assert e._lib.oaz_selfplay_step(e.handle, 1) == _abi.ERR_STATE
        e.set_search_time(0.0)
        # oaz_search ignores the cap
        r = e.search(roots)
        assert r.moves.tobytes() == want.moves.tobytes() and r.pi.tobytes() == want.pi.tobytes()
        assert r.stats.sims == 8 * SIMS and e.tree(3).tobytes() == want_tree.tobytes()
        e.selfplay_step(2)
        full, fastp = e.playout_cap_stats()
        assert full + fastp == e.selfplay_stats().moves == 16
        # cleared: the engine plays as one that never had a cap
        e.set_playout_cap(0, 0)
        assert e.playout_cap_stats() == (0, 0)
        e.selfplay_step(3)  # (from a reset: changing the cap ended the running games)
        st = e.selfplay_stats()
        assert st.moves == want_plies == 24 and st.search.sims == 24 * SIMS
        assert e.playout_cap_stats() == (0, 0)


def test_c7_one_training_iteration(tmp_path):
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train

    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=1),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=16, train=True), iterations=1,
                     training_epochs=1, train_batch_size=16, self_play_game_amnt=64, save_checkpoint=99,
                     evaluation_checkpoint=99, max_plies=20, playout_cap_fast_sims=4, playout_cap_full=16384)
    st = train(cfg, folder=str(tmp_path / "capped"))
    assert st.iteration == [1] and np.isfinite(st.loss[0])
    g = st.games_played[-1]
    assert g["games_amnt"] == 64
    assert g["plies_played"] > g["positions_retrieved"] > 0
