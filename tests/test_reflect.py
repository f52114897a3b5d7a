"""CPU: the left-right reflection (include/onitama_az.h, "left-right reflection").

The card map against the attack maps, the host entries against the numpy restatement (reflect_util), the law
itself on the oracle's rules (the reference's rules as the oracle restates them commute with the reflection:
masks, move lists, make_move, current_state, encode), and the epoch drivers' index and flag streams against a
recording stub trainer. Nothing here needs a GPU.
"""
import numpy as np
import pytest

import reflect_util as ru
from onitama_az import _abi
from onitama_az import game
from onitama_az import trainer as trn

N_PLAY, SEED = 5000, 20261021


@pytest.fixture(scope="module")
def play(orc):
    return ru.random_play(orc, N_PLAY, SEED)


# ---- card map -----------------------------------------------------------------------------------------
def test_card_map_follows_from_the_attack_maps(lib):
    att = np.zeros((2, 16, 25), dtype=np.uint32)
    lib.oaz_attack_maps(_abi.ptr(att))
    derived = ru.card_map_from_attack(att)
    assert all(len(c) == 1 for c in derived), derived  # the law names exactly one card
    cmap = [c[0] for c in derived]
    assert cmap == ru.CARDS == [lib.oaz_reflect_card(k) for k in range(16)] == [game.reflect_card(k) for k in range(16)]
    assert all(cmap[cmap[k]] == k for k in range(16))
    assert sum(cmap[k] == k for k in range(16)) == 8
    assert sorted((k, cmap[k]) for k in range(16) if k < cmap[k]) == [(2, 3), (6, 7), (11, 12), (14, 15)]
    assert lib.oaz_reflect_card(-1) == -1 and lib.oaz_reflect_card(16) == -1
    assert game.reflect_card(game.FROG) is game.RABBIT and game.reflect_card(game.TIGER) is game.TIGER
    assert [game.reflect_square(i) for i in (0, 2, 4, 5, 12, 24, 25)] == [4, 2, 0, 9, 12, 20, 25]
    assert [game.reflect_square(i) for i in range(26)] == [ru.R(i) for i in range(26)]


# ---- host entries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_host_entries_equal_the_restatement(lib, play, n):
    samples = ru.random_samples(play, n, seed=n + 1)
    samples["state"]["pad"] = np.random.default_rng(n).integers(0, 256, (n, 2))  # pad travels unchanged
    states = np.ascontiguousarray(samples["state"])
    moves = play.moves[:n].copy()
    if n:
        moves[0] = (25, 25, 0, 1)  # the pass move
    for fn, a, ref in ((lib.oaz_reflect_states_host, states, ru.reflect_states(states)),
                       (lib.oaz_reflect_moves_host, moves, ru.reflect_moves(moves)),
                       (lib.oaz_reflect_samples_host, samples, ru.reflect_samples(samples))):
        out = np.zeros(max(n, 1), dtype=a.dtype)
        assert fn(_abi.ptr(a if n else out), n, _abi.ptr(out)) == 0
        if n == 0:
            assert out.tobytes() == bytes(out.nbytes)  # nothing written
            continue
        assert out.tobytes() == ref.tobytes()
        back = np.zeros_like(a)
        assert fn(_abi.ptr(out), n, _abi.ptr(back)) == 0 and back.tobytes() == a.tobytes()  # twice: the bytes again
        inplace = a.copy()
        assert fn(_abi.ptr(inplace), n, _abi.ptr(inplace)) == 0 and inplace.tobytes() == ref.tobytes()
    if n:
        assert np.array_equal(ru.reflect_states(states)["pad"], states["pad"]) and states["pad"].any()
        got = game.reflect_moves(moves)
        assert tuple(got[0]) == (25, 25, 0, 1)  # the pass move is a fixed point
        assert game.reflect_samples(samples).tobytes() == ru.reflect_samples(samples).tobytes()
        assert game.reflect_states(states).tobytes() == ru.reflect_states(states).tobytes()


def test_python_objects_reflect(play):
    st, colour = game.State.from_np(play.states[7])
    ref, _ = game.State.from_np(ru.reflect_states(play.states[7:8])[0])
    r = st.reflected()
    assert (r.kings, r.pawns, r.deck.indices()) == (ref.kings, ref.pawns, ref.deck.indices())
    rr = r.reflected()
    assert (rr.kings, rr.pawns, rr.deck.indices()) == (st.kings, st.pawns, st.deck.indices())
    mv = game.DoneMove(game.Move(0, 6, game.PieceKind.King), 3).reflected()
    assert (mv.mov.from_, mv.mov.to, mv.mov.piece, mv.used_card_idx) == (4, 8, game.PieceKind.King, 3)
    with pytest.raises(ValueError):
        game.reflect_square(26)


def test_host_entries_reject_bad_cards_and_squares(lib, play):
    n = 8
    samples = ru.random_samples(play, n, seed=3)
    bad = samples.copy()
    bad["state"]["cards"][5][4] = 16
    fill = np.full(n, 0x5A, dtype=np.uint8).repeat(_abi.SAMPLE_DTYPE.itemsize).view(_abi.SAMPLE_DTYPE)
    out = fill.copy()
    assert lib.oaz_reflect_samples_host(_abi.ptr(bad), n, _abi.ptr(out)) == _abi.ERR_ARG
    assert out.tobytes() == fill.tobytes()
    st, sout = np.ascontiguousarray(bad["state"]), np.ascontiguousarray(fill["state"])
    assert lib.oaz_reflect_states_host(_abi.ptr(st), n, _abi.ptr(sout)) == _abi.ERR_ARG
    assert sout.tobytes() == np.ascontiguousarray(fill["state"]).tobytes()
    for field in ("from_", "to"):
        mv = play.moves[:n].copy()
        mv[field][n - 1] = 26
        mout = np.full(n * 4, 0x5A, dtype=np.uint8).view(_abi.MOVE_DTYPE)
        assert lib.oaz_reflect_moves_host(_abi.ptr(mv), n, _abi.ptr(mout)) == _abi.ERR_ARG
        assert mout.tobytes() == b"\x5A" * (4 * n)
    # in place, too: the input stays
    keep = bad.copy()
    assert lib.oaz_reflect_samples_host(_abi.ptr(bad), n, _abi.ptr(bad)) == _abi.ERR_ARG and bad.tobytes() == keep.tobytes()
    # the GPU entry checks its arguments before it looks for a device
    assert lib.oaz_reflect_samples(_abi.ptr(bad), n, _abi.ptr(out)) == _abi.ERR_ARG and out.tobytes() == fill.tobytes()


# ---- the law, on the oracle's rules ------------------------------------------------------------------------
def test_oracle_rules_commute_with_the_reflection(orc, play):
    assert len(play.states) >= 5000
    ru.assert_both_colours_capture_and_win(play)
    rs, rm, ra = ru.reflect_states(play.states), ru.reflect_moves(play.moves), ru.reflect_states(play.after)
    enc = np.zeros((len(play.states), 21, 5, 5), dtype=np.float32)
    renc = np.zeros_like(enc)
    for i in range(len(play.states)):
        s, r = play.states[i:i + 1], rs[i:i + 1]
        masks, rmasks = orc.movegen_masks(s), orc.movegen_masks(r)
        for k in range(2):
            for f in range(25):
                m = int(masks[k][f])  # (mostly 0: no own piece on f)
                assert (ru.reflect_board(m) if m else 0) == int(rmasks[k][ru.R(f)]), (i, k, f)
        legal = orc.movegen(s)
        # as sets: the reference lists moves by ascending `from`, which the reflection reorders inside a row
        assert ru.move_set(ru.reflect_moves(legal)) == ru.move_set(orc.movegen(r)), i
        nxt = r.copy()
        m = rm[i]
        res = orc.make_move(nxt, tuple(int(m[k]) for k in ("from_", "to", "piece", "slot")), int(nxt["to_move"][0]))
        nxt["to_move"][0] ^= 1
        assert res == play.results[i] and nxt.tobytes() == ra[i:i + 1].tobytes(), i
        assert orc.current_state(s) == orc.current_state(r), i
        assert orc.current_state(play.after[i:i + 1]) == orc.current_state(ra[i:i + 1]), i
        enc[i], renc[i] = orc.encode(s), orc.encode(r)
    assert np.array_equal(renc, ru.reflect_planes(enc))
    assert np.array_equal(renc[:, :4], enc[:, :4, :, ::-1]) and np.array_equal(renc[:, 20], enc[:, 20])
    assert np.any(renc[:, 4:20] != enc[:, 4:20])  # some card plane did move


# ---- epoch drivers ---------------------------------------------------------------------------------------
class StubTrainer:
    """Records what the epoch drivers upload."""

    def __init__(self):
        self.uploads = []

    def load_samples(self, samples):
        self.n = len(samples)

    def set_batches(self, idx, reflect=None):
        self.uploads.append((np.array(idx, dtype=np.int32), None if reflect is None else np.array(reflect)))
        self.k = len(idx)

    def train(self, first, count):
        assert (first, count) == (0, self.k)

    def losses(self):
        return 2.0 * self.k, 4.0 * self.k, self.k


def _uploads(reflect, n=100, batch=16, epochs=3, seed=11, **kw):
    tr = StubTrainer()
    hist = trn.train_epochs(tr, np.zeros(n, dtype=_abi.SAMPLE_DTYPE), epochs=epochs, batch=batch, seed=seed,
                            **({} if reflect is None else {"reflect": reflect}), **kw)
    assert len(hist) == epochs == len(tr.uploads)
    return tr.uploads


def test_reflect_off_uploads_the_index_stream_of_the_seed():
    rng = np.random.default_rng(11)
    want = [trn.choose_batches(rng, 100, 16, 100 // 16) for _ in range(3)]
    for reflect in (None, 0, 1):  # mode 1 leaves the index stream and the epoch length alone, too
        got = _uploads(reflect)
        assert all(np.array_equal(g[0], w) for g, w in zip(got, want)), reflect
        assert all((g[1] is None) == (reflect != 1) for g in got)


def test_flags_are_reproducible_from_the_seed_and_their_own_stream():
    a, b, c = _uploads(1), _uploads(1), _uploads(1, seed=12)
    for (ia, fa), (ib, fb) in zip(a, b):
        assert np.array_equal(fa, fb) and fa.shape == ia.shape and fa.dtype == np.uint8
    flags = np.concatenate([f.reshape(-1) for _, f in a])
    assert set(flags.tolist()) == {0, 1} and 0.3 < flags.mean() < 0.7  # 288 fair draws
    assert any(not np.array_equal(fa, fc) for (_, fa), (_, fc) in zip(a, c))
    frng = np.random.default_rng([trn.REFLECT_TAG, 11])
    assert np.array_equal(a[0][1], trn.choose_reflect(frng, (6, 16)))


def test_mode_two_draws_from_the_doubled_buffer():
    n, batch = 100, 16
    got = _uploads(2)
    rng = np.random.default_rng(11)
    for idx, flags in got:
        assert idx.shape == flags.shape == (2 * n // batch, batch)
        assert idx.min() >= 0 and idx.max() < n and set(np.unique(flags).tolist()) == {0, 1}
        for row_i, row_f in zip(idx, flags):
            assert len({(int(i), int(f)) for i, f in zip(row_i, row_f)}) == batch  # no (sample, flag) pair twice
        virt = trn.choose_batches(rng, 2 * n, batch, 2 * n // batch)  # choose_multiple over the doubled buffer
        assert np.array_equal(idx + n * flags, virt)
    with pytest.raises(ValueError):
        _uploads(3)


@pytest.mark.parametrize("reflect", [0, 1, 2])
def test_data_parallel_slices_of_flags_and_indices_line_up(reflect):
    n, batch, world, seed = 100, 32, 2, 5

    def draw(rank, world):
        rng, frng = np.random.default_rng(seed), np.random.default_rng([trn.REFLECT_TAG, seed])
        return [trn.epoch_batches(rng, frng, n, batch, reflect, rank, world) for _ in range(2)]

    whole, parts = draw(0, 1), [draw(r, world) for r in range(world)]
    for e, (idx, flags) in enumerate(whole):
        assert np.array_equal(np.hstack([parts[r][e][0] for r in range(world)]), idx)
        assert all(parts[r][e][0].shape == (len(idx), batch // world) for r in range(world))
        if reflect == 0:
            assert flags is None and all(parts[r][e][1] is None for r in range(world))
        else:
            assert np.array_equal(np.hstack([parts[r][e][1] for r in range(world)]), flags)
