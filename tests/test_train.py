"""Training step: oaz_trainer_* against oracle/train_ref.py, a float64
torch-CPU restatement of net.rs forward(train=true) + alphaloss + tch SGD (train.rs:264-313).

Tolerances (fp32 GPU vs fp64 CPU): gradients within 2e-4 x the tensor's max |g| (+1e-7), losses
within 1e-5 relative, parameters / running stats within 1e-6 + 1e-5 relative after the step.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

from onitama_az import _abi
from onitama_az.weights import named_from_blob
from train_util import _batch, _close_grads, _close_params, _run_steps, _weights  # noqa: F401

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))


# ---- CPU: the restatement itself ------------------------------------------------------------------
def test_reference_loss_quirks():
    import torch
    from train_ref import alphaloss
    v = torch.tensor([[0.5], [-0.25], [0.0]], dtype=torch.float64)
    z = torch.tensor([1.0, -1.0, 0.0], dtype=torch.float64)
    lv, _ = alphaloss(v, torch.full((3, 2, 25), 0.02, dtype=torch.float64), torch.zeros(3, 2, 25, dtype=torch.float64),
                      z, broadcast=True)
    ref = np.mean([(zj - vi) ** 2 for vi in (0.5, -0.25, 0.0) for zj in (1.0, -1.0, 0.0)])  # [B,B] broadcast
    assert abs(float(lv) - ref) < 1e-12
    lv2, _ = alphaloss(v, torch.full((3, 2, 25), 0.02, dtype=torch.float64), torch.zeros(3, 2, 25, dtype=torch.float64),
                       z, broadcast=False)
    assert abs(float(lv2) - np.mean([(1 - 0.5) ** 2, (-1 + 0.25) ** 2, 0.0])) < 1e-12
    p = torch.full((2, 2, 25), 1 / 50, dtype=torch.float64)
    pi = torch.zeros(2, 2, 25, dtype=torch.float64)
    pi[:, 0, 0] = 1.0
    _, lp = alphaloss(torch.zeros(2, 1, dtype=torch.float64), p, pi, torch.zeros(2, dtype=torch.float64))
    assert abs(float(lp) - np.log(50) / 25) < 1e-12  # sum over dim 1, mean over B*25


def test_choose_batches_without_replacement():
    from onitama_az.trainer import choose_batches
    idx = choose_batches(np.random.default_rng(0), 1000, 512, 3)
    assert idx.shape == (3, 512) and idx.dtype == np.int32
    for row in idx:
        assert len(set(row.tolist())) == 512 and row.min() >= 0 and row.max() < 1000


def test_trainer_without_device_is_a_loud_error(lib):
    if _abi.device_count() > 0:
        pytest.skip("a GPU is visible")
    from onitama_az.trainer import Trainer
    with pytest.raises(_abi.OazError, match="device"):
        Trainer(blocks=3)


def test_reference_optimiser_equals_torch_sgd(orc):
    """train_step's optimiser against torch.optim.SGD(momentum=, weight_decay=) stepping the same float64
    parameters from the same gradients, at non-default lr / momentum / weight decay: three steps, 1e-12.
    The hyperparameter cases of tests/test_gpu_train.py lean on this half of the restatement."""
    import torch
    from train_ref import RUNNING, train_step
    blocks, B, steps, lr, mom, wd = 1, 16, 3, 0.03, 0.7, 2e-3
    samples, planes = _batch(orc, B * steps, 21)
    named = {k: np.asarray(v, dtype=np.float64) for k, v in named_from_blob(_weights(21, blocks), blocks).items()}
    params = {k: torch.tensor(v, requires_grad=True) for k, v in named.items() if not k.endswith(RUNNING)}
    opt = torch.optim.SGD(list(params.values()), lr=lr, momentum=mom, weight_decay=wd)
    bufs = None
    for s in range(steps):
        rows = slice(s * B, (s + 1) * B)
        named, grads, _, _, bufs = train_step(named, planes[rows], samples["pi"][rows], samples["z"][rows], blocks,
                                              lr=lr, momentum=mom, wd=wd, bufs=bufs)
        for k, t in params.items():
            t.grad = torch.tensor(grads[k])
        opt.step()
        for k, t in params.items():
            assert np.abs(t.detach().numpy() - named[k]).max() <= 1e-12, (s, k)


def test_reference_float32_mode_inside_project_bars(orc):
    """The restatement in float32 against itself in float64 on the _batch / _weights inputs (blocks 2,
    B 32) stays inside the project's bars: the bars are reachable by a correct fp32 implementation."""
    from train_ref import train_step
    blocks, B = 2, 32
    samples, planes = _batch(orc, B, 5)
    named = named_from_blob(_weights(5, blocks), blocks)
    p64, g64, lv64, lp64, _ = train_step(named, planes, samples["pi"], samples["z"], blocks)
    p32, g32, lv32, lp32, _ = train_step(named, planes, samples["pi"], samples["z"], blocks, dtype=np.float32)
    assert all(g.dtype == np.float32 for g in g32.values()) and all(g.dtype == np.float64 for g in g64.values())
    _close_grads(g32, g64)
    assert abs(lv32 - lv64) <= 1e-5 * abs(lv64) and abs(lp32 - lp64) <= 1e-5 * abs(lp64), (lv32, lv64, lp32, lp64)
    _close_params(p32, p64)


# ---- GPU parity ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_train_step_matches_reference_restatement(orc):
    _run_steps(orc, blocks=3, B=64, steps=1)


@pytest.mark.gpu
def test_train_two_steps_momentum(orc):
    _run_steps(orc, blocks=2, B=32, steps=2, seed=5)


@pytest.mark.gpu
def test_train_step_elementwise_value_loss(orc):
    _run_steps(orc, blocks=1, B=16, steps=1, broadcast=False, seed=7)


@pytest.mark.gpu
def test_train_step_reference_batch_512(orc):
    _run_steps(orc, blocks=3, B=512, steps=1, seed=9)


@pytest.mark.gpu
def test_train_epochs_reduce_loss(orc):
    from onitama_az.trainer import Trainer, train_epochs
    samples, _ = _batch(orc, 1024, 11)
    with Trainer(blocks=2, max_batch=128, learning_rate=2e-2) as tr:
        tr.set_weights(_weights(11, 2))
        hist = train_epochs(tr, samples, epochs=6, batch=128, seed=0)
    assert len(hist) == 6 and all(h.steps == 8 for h in hist)
    assert hist[-1].loss < hist[0].loss, [h.loss for h in hist]


@pytest.mark.gpu
def test_alphazero_loop_end_to_end(tmp_path):
    """train.rs:158-412 in miniature: self-play -> SGD epochs -> pit -> checkpoints."""
    import json
    import os
    from onitama_az.evaluator import EvaluatorConfig
    from onitama_az.mcts import AlphaZeroMctsConfig, ConvResNetConfig
    from onitama_az.train_loop import LoopConfig, train
    from onitama_az.weights import blob_from_named, read_ot
    cfg = LoopConfig(model_config=ConvResNetConfig(resnet_block_amnt=1),
                     mcts_config=AlphaZeroMctsConfig(exploration_c=5.0, max_playouts=8, train=True),
                     iterations=2, training_epochs=2, train_batch_size=32, self_play_game_amnt=16,
                     save_checkpoint=2, evaluation_checkpoint=1, max_plies=40,
                     evaluator_config=EvaluatorConfig(game_amnt=2, max_plies=20, seed=3))
    st = train(cfg, folder=str(tmp_path), eval_sims=8)
    assert st.iteration == [1, 2] and len(st.fight_statistics) == 2
    assert all(g["positions_retrieved"] > 32 for g in st.games_played)
    assert all(np.isfinite(st.loss))
    files = os.listdir(tmp_path)
    ckpt = [f for f in files if f.startswith("model_2_") and f.endswith(".ot")]
    assert ckpt and "stats.json" in files
    w = blob_from_named(read_ot(str(tmp_path / ckpt[0])), 1)
    assert w.size == 240006 - 2 * 2 * (64 * 64 * 9 + 64 * 5)
    json.load(open(tmp_path / "stats.json"))
