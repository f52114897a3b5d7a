"""Trainer: the training half of the AlphaZero loop on the GPU.

Mirrors the body of `train()` (alphazero-training/src/train.rs:264-339): for each epoch,
`train_amnt = len(buffer) // batch` batches drawn with `choose_multiple` (a uniform draw without
replacement; seeded numpy here, the reference uses thread_rng), each one
`forward(train=true) -> alphaloss -> opt.backward_step` with nn::Sgd{momentum 0.9} and
weight decay l2_const (train.rs:181-186). Every step runs in libonitama_az.so
(oaz_trainer_*, csrc/oaz_train.hip); this module only draws indices and keeps statistics.

Data-parallel training (`world > 1`, train_epochs_dp): every rank runs backward on its own batch
shard, the flat gradient buffer is all-reduced (the C ABI's RCCL communicator, oaz_comm_*) on the
trainer's stream, then every rank applies the same SGD step (grad_scale = 1/world); BN running
statistics and losses are averaged over ranks after each epoch.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _abi


@dataclass
class EpochLoss:  # the per-epoch line of train.rs:316-324
    loss: float
    value: float
    policy: float
    steps: int


@dataclass
class EvalStats:
    """oaz_eval_stats: sums over the entries of one Trainer.evaluate call (the network in eval mode, every BN on its
    running statistics), and the means a reader wants of them. All means are 0.0 over no entries."""
    n: int = 0
    decided: int = 0  # entries with z != 0
    top1: int = 0  # entries whose arg-max prior is a largest entry of pi
    sign: int = 0  # decided entries with v z > 0
    value_sq_sum: float = 0.0  # sum (z - v)^2, elementwise
    policy_ce_sum: float = 0.0  # sum of -sum_k pi_k log p_k
    target_entropy_sum: float = 0.0  # sum of -sum_k pi_k log pi_k

    def _per(self, x: float, d: float) -> float:
        return x / d if d else 0.0

    @property
    def value_mse(self) -> float:
        return self._per(self.value_sq_sum, self.n)

    @property
    def policy_ce(self) -> float:
        return self._per(self.policy_ce_sum, self.n)

    @property
    def policy_kl(self) -> float:
        return self._per(self.policy_ce_sum - self.target_entropy_sum, self.n)

    @property
    def top1_rate(self) -> float:
        return self._per(self.top1, self.n)

    @property
    def sign_rate(self) -> float:
        return self._per(self.sign, self.decided)

    @property
    def policy_loss(self) -> float:
        """policy_ce_sum / (25 n): the unit of EpochLoss.policy (alphaloss's mean over B x 25 entries)."""
        return self._per(self.policy_ce_sum, 25 * self.n)

    def summary(self) -> dict:
        """The counts and the means as one JSON-ready dict (Stats.evaluation)."""
        return {"n": self.n, "decided": self.decided, "value_mse": self.value_mse, "policy_ce": self.policy_ce,
                "policy_kl": self.policy_kl, "policy_loss": self.policy_loss, "top1_rate": self.top1_rate,
                "sign_rate": self.sign_rate}


class Trainer:
    def __init__(self, blocks: int, max_batch: int = 512, learning_rate: float = 5e-3, momentum: float = 0.9,
                 weight_decay: float = 1e-4, value_loss_broadcast: bool = True, device: int = 0,
                 bn_momentum: Optional[float] = None, bn_eps: Optional[float] = None):
        lib = _abi.load()
        cfg = _abi.oaz_train_config()
        lib.oaz_train_config_default(C.byref(cfg))
        cfg.blocks, cfg.max_batch = int(blocks), int(max_batch)
        cfg.learning_rate, cfg.momentum, cfg.weight_decay = learning_rate, momentum, weight_decay
        if bn_momentum is not None:  # None: the config's own default (tch's 0.1 / 1e-5)
            cfg.bn_momentum = bn_momentum
        if bn_eps is not None:
            cfg.bn_eps = bn_eps
        cfg.value_loss_broadcast = int(bool(value_loss_broadcast))
        h = lib.oaz_trainer_create(C.byref(cfg), int(device))
        if not h:
            raise _abi.OazError(f"oaz_trainer_create failed: {lib.oaz_last_error().decode()}")
        self._h, self._lib, self.config, self.device = C.c_void_p(h), lib, cfg, device
        self.blocks = int(blocks)
        self.n_params = int(lib.oaz_weight_count(self.blocks, 64, 21))
        self.n_samples = 0

    def close(self) -> None:
        if self._h:
            self._lib.oaz_trainer_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        _abi.check(rc)

    # -- parameters ---------------------------------------------------------------------------
    def set_weights(self, blob: np.ndarray) -> None:
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(self._lib.oaz_trainer_set_weights(self._h, _abi.ptr(blob), blob.size))

    def get_weights(self) -> np.ndarray:
        out = np.zeros(self.n_params, dtype=np.float32)
        self._check(self._lib.oaz_trainer_get_weights(self._h, _abi.ptr(out), out.size))
        return out

    def save_ot(self, path: str) -> None:
        """The training weights as a .ot checkpoint (oaz_trainer_save_ot; save_vs, train.rs:414-430)."""
        self._check(self._lib.oaz_trainer_save_ot(self._h, str(path).encode()))

    def grads(self) -> np.ndarray:
        out = np.zeros(self.n_params, dtype=np.float32)
        self._check(self._lib.oaz_trainer_get_grads(self._h, _abi.ptr(out), out.size))
        return out

    def grads_device(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.oaz_trainer_grads(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def set_stream(self, stream_handle: Optional[int]) -> None:
        self._check(self._lib.oaz_trainer_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    # -- data ------------------------------------------------------------------------------------
    def load_samples(self, samples: np.ndarray) -> None:
        samples = np.ascontiguousarray(samples, dtype=_abi.SAMPLE_DTYPE)
        self._check(self._lib.oaz_trainer_load_samples(self._h, _abi.ptr(samples), len(samples)))
        self.n_samples = len(samples)

    def bind_device_samples(self, dev_ptr: int, n: int) -> None:
        self._check(self._lib.oaz_trainer_bind_device_samples(self._h, C.c_void_p(dev_ptr), int(n)))
        self.n_samples = int(n)

    def set_batches(self, idx: np.ndarray, reflect: Optional[np.ndarray] = None) -> None:
        """Upload the index matrix [n_batches, batch]. reflect (same shape, 0 / 1; None = all 0): a flagged entry
        stands for the left-right reflected sample (oaz_trainer_set_batches_reflect): the step's gather produces its
        planes, pi and z, with no copy of the buffer."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.ndim == 2
        if reflect is None:
            self._check(self._lib.oaz_trainer_set_batches(self._h, _abi.ptr(idx), idx.shape[0], idx.shape[1]))
            return
        reflect = np.ascontiguousarray(reflect, dtype=np.uint8)
        assert reflect.shape == idx.shape
        self._check(self._lib.oaz_trainer_set_batches_reflect(self._h, _abi.ptr(idx), _abi.ptr(reflect), idx.shape[0],
                                                              idx.shape[1]))

    # -- steps -------------------------------------------------------------------------------------
    def backward(self, b: int) -> None:
        self._check(self._lib.oaz_trainer_backward(self._h, int(b)))

    def apply(self, grad_scale: float = 1.0) -> None:
        self._check(self._lib.oaz_trainer_apply(self._h, C.c_float(grad_scale)))

    def train(self, first: int, count: int) -> None:
        self._check(self._lib.oaz_trainer_train(self._h, int(first), int(count)))

    def losses(self) -> Tuple[float, float, int]:
        """(sum of value losses, sum of policy losses, steps) since the previous call."""
        out = (C.c_double * 3)()
        self._check(self._lib.oaz_trainer_losses(self._h, C.byref(out)))
        return float(out[0]), float(out[1]), int(out[2])

    def sync(self) -> None:
        self._check(self._lib.oaz_trainer_sync(self._h))

    # -- the eval-mode pass ------------------------------------------------------------------------
    def _entries(self, idx, reflect):
        """(idx int32 or None, n, reflect uint8 or None) of evaluate / predict: idx None = every sample."""
        if idx is None:
            n = int(self.n_samples)
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
            n = len(idx)
        if reflect is not None:
            reflect = np.ascontiguousarray(reflect, dtype=np.uint8).reshape(-1)
            assert len(reflect) == n
        return idx, n, reflect

    def evaluate(self, idx: Optional[np.ndarray] = None, reflect: Optional[np.ndarray] = None) -> EvalStats:
        """The network in eval mode (every BN on its running statistics) over samples[idx] (None: all of the loaded
        or bound samples); reflect: a flag per entry, as set_batches'. oaz_trainer_evaluate: nothing a training step
        reads or reports changes, and the sums are the same bytes for every max_batch."""
        idx, n, reflect = self._entries(idx, reflect)
        st = _abi.oaz_eval_stats()
        self._check(self._lib.oaz_trainer_evaluate(self._h, None if idx is None else _abi.ptr(idx), n,
                                                   None if reflect is None else _abi.ptr(reflect), C.byref(st)))
        return EvalStats(int(st.n), int(st.decided), int(st.top1), int(st.sign), float(st.value_sq),
                         float(st.policy_ce), float(st.target_entropy))

    def predict(self, idx: Optional[np.ndarray] = None,
                reflect: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(p [n, 50], v [n]) float32 of the same pass (oaz_trainer_predict); a flagged entry's p is in the
        reflected coordinates."""
        idx, n, reflect = self._entries(idx, reflect)
        p, v = np.zeros((n, 50), dtype=np.float32), np.zeros(n, dtype=np.float32)
        self._check(self._lib.oaz_trainer_predict(self._h, None if idx is None else _abi.ptr(idx), n,
                                                  None if reflect is None else _abi.ptr(reflect), _abi.ptr(p),
                                                  _abi.ptr(v)))
        return p, v


def choose_batches(rng: np.random.Generator, n_samples: int, batch: int, n_batches: int) -> np.ndarray:
    """`data_buffer.iter().choose_multiple(&mut rng, batch)` per batch (train.rs:272-276): a uniform
    draw without replacement inside a batch, independent across batches."""
    return np.stack([rng.choice(n_samples, size=batch, replace=False) for _ in range(n_batches)]).astype(np.int32)


REFLECT_TAG = 0x5245464C  # "REFL": the reflect flags' generator is default_rng([REFLECT_TAG, seed])


def choose_reflect(rng: np.random.Generator, shape) -> np.ndarray:
    """Mode 1's flags: every entry 0 or 1 with probability 1/2 each (uint8, `shape`)."""
    return rng.integers(0, 2, size=shape, dtype=np.uint8)


def choose_batches_doubled(rng: np.random.Generator, n_samples: int, batch: int,
                           n_batches: int) -> Tuple[np.ndarray, np.ndarray]:
    """Mode 2's draw: `choose_batches` over the 2 n virtual entries of the buffer together with its reflection,
    entry j >= n being sample j - n reflected; returns (index matrix, flag matrix). The doubled buffer is never
    made: no batch holds the same (sample, flag) pair twice, and may hold a sample and its reflection."""
    virt = choose_batches(rng, 2 * n_samples, batch, n_batches)
    return (virt % n_samples).astype(np.int32), (virt >= n_samples).astype(np.uint8)


def epoch_batches(rng: np.random.Generator, flag_rng: np.random.Generator, n_samples: int, batch: int,
                  reflect: int, rank: int = 0, world: int = 1,
                  subset: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """One epoch's (index matrix, flag matrix or None) for `reflect` (train_epochs). rng is the index generator and
    flag_rng the flags' own: mode 0 and 1 draw from rng exactly what the loop without the feature draws. world > 1
    (train_epochs_dp): every rank draws the whole matrices and gets its batch / world columns of both."""
    if reflect not in (0, 1, 2):
        raise ValueError("reflect is 0 (off), 1 (each entry with probability 1/2) or 2 (the doubled buffer)")
    if reflect == 2:
        idx, flags = choose_batches_doubled(rng, n_samples, batch, 2 * n_samples // batch)
    else:
        idx = choose_batches(rng, n_samples, batch, n_samples // batch)
        flags = choose_reflect(flag_rng, idx.shape) if reflect == 1 else None
    if subset is not None:
        idx = subset[idx]
    cols = slice(rank * (batch // world), (rank + 1) * (batch // world))
    return idx[:, cols], (None if flags is None else flags[:, cols])


def _subset(subset, n_samples: int) -> Tuple[Optional[np.ndarray], int]:
    """(the subset as int32 or None, the number of entries an epoch draws from)."""
    if subset is None:
        return None, int(n_samples)
    subset = np.ascontiguousarray(subset, dtype=np.int32).reshape(-1)
    if len(subset) and (subset.min() < 0 or subset.max() >= n_samples):
        raise ValueError("subset: an index outside the samples")
    return subset, len(subset)


def _set_batches(trainer, idx, flags) -> None:
    if flags is None:
        trainer.set_batches(idx)
    else:
        trainer.set_batches(idx, flags)


def train_epochs(trainer: Trainer, samples: np.ndarray, epochs: int = 10, batch: int = 512,
                 seed: int = 0, reflect: int = 0, subset: Optional[np.ndarray] = None) -> List[EpochLoss]:
    """The epoch loop of train.rs:264-325 on one GPU (stops early, as the reference, when the
    buffer holds fewer than `batch` samples).

    reflect: training on the left-right reflected records too (include/onitama_az.h, "left-right reflection"; the
    reference does not). 0 = off: the index stream of a seed is what it always was. 1 = every drawn entry is
    reflected with probability 1/2, the flags from a generator of their own (seed and REFLECT_TAG), the index
    stream and the epoch length unchanged. 2 = the buffer together with its reflection: every batch a draw
    without replacement from the 2 n entries, 2 n // batch batches per epoch.

    subset (sample indices; None = all, the index and flag streams of a seed then being what they were): training
    draws from these samples only (the rest are held out, onitama_az.holdout): a batch is
    subset[choose_batches(rng, len(subset), ...)], an epoch len(subset) // batch batches, and mode 2 draws from
    2 len(subset) virtual entries."""
    trainer.load_samples(samples)
    return _epochs(trainer, len(samples), epochs, batch, seed, reflect, subset)


def train_epochs_device(trainer: Trainer, ptr: int, n: int, epochs: int = 10, batch: int = 512, seed: int = 0,
                        reflect: int = 0, subset: Optional[np.ndarray] = None) -> List[EpochLoss]:
    """train_epochs on n records that are already in device memory at `ptr` (a ReplayBuffer view; the trainer's
    device): they are bound (oaz_trainer_bind_device_samples), never copied, and the index and flag streams are
    those train_epochs draws for the same n, seed and reflect. The memory stays the caller's and stays as it is
    until the call returns."""
    trainer.bind_device_samples(ptr, n)
    return _epochs(trainer, int(n), epochs, batch, seed, reflect, subset)


def _epochs(trainer, n_samples: int, epochs: int, batch: int, seed: int, reflect: int,
            subset: Optional[np.ndarray] = None) -> List[EpochLoss]:
    """The epochs of train_epochs on the samples the trainer holds."""
    subset, n_samples = _subset(subset, n_samples)
    rng = np.random.default_rng(seed)
    flag_rng = np.random.default_rng([REFLECT_TAG, seed])
    out: List[EpochLoss] = []
    for _ in range(epochs):
        if n_samples < batch:
            break
        idx, flags = epoch_batches(rng, flag_rng, n_samples, batch, reflect, subset=subset)
        n = len(idx)
        _set_batches(trainer, idx, flags)
        trainer.train(0, n)
        v, p, k = trainer.losses()
        out.append(EpochLoss((v + p) / k, v / k, p / k, k))
    return out


class _DeviceArray:
    """Zero-copy view of a device buffer for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3,
                                         "strides": None}


def _allreduce_sum(t, comm, stream: int) -> None:
    """Sum over ranks in place: the C ABI's RCCL communicator on `stream`, or (no comm: gloo CPU
    tests / one-GPU rehearsals) torch.distributed through a host copy."""
    import torch
    import torch.distributed as dist
    if comm is not None:
        comm.allreduce_sum_(t, stream)
        return
    torch.cuda.current_stream().synchronize()
    h = t.cpu()
    dist.all_reduce(h)
    t.copy_(h.to(t.device))


def train_epochs_dp(trainer: Trainer, samples: np.ndarray, epochs: int, batch: int, seed: int, rank: int,
                    world: int, comm=None, reflect: int = 0, subset: Optional[np.ndarray] = None) -> List[EpochLoss]:
    """Data-parallel epochs (train.rs:264-325 over `world` GPUs): the global batch `batch` is split
    into `world` shards of batch/world samples; the gradient buffer is summed over ranks (RCCL via
    `comm`, an onitama_az.dist.Comm) and applied with grad_scale 1/world, so every rank takes the
    same SGD step. All ranks draw the same index stream (same seed, same gathered `samples`) and take
    their shard. BN batch statistics are per shard (DDP without SyncBatchNorm); the running
    statistics are averaged over ranks after each epoch, and the reported losses are the global
    ones, so every rank ends each epoch with identical weights and statistics. reflect: as train_epochs; every
    rank draws the same flags and takes the column slice of them that it takes of the indices. subset: as
    train_epochs, the same on every rank."""
    return _dp(trainer, lambda: trainer.load_samples(samples), len(samples), epochs, batch, seed, rank, world, comm,
               reflect, subset)


def train_epochs_dp_device(trainer: Trainer, ptr: int, n: int, epochs: int, batch: int, seed: int, rank: int,
                           world: int, comm=None, reflect: int = 0,
                           subset: Optional[np.ndarray] = None) -> List[EpochLoss]:
    """train_epochs_dp on n records bound in device memory (train_epochs_device's terms): every rank binds its own
    copy of the same records."""
    return _dp(trainer, lambda: trainer.bind_device_samples(ptr, n), int(n), epochs, batch, seed, rank, world, comm,
               reflect, subset)


def _dp(trainer, attach, n_samples, epochs, batch, seed, rank, world, comm, reflect, subset=None) -> List[EpochLoss]:
    import torch
    assert batch % world == 0 and (batch // world) % 16 == 0
    shard = batch // world
    # one explicit stream for the trainer's kernels, the collectives and the torch copies (the legacy
    # default stream, handle 0, would mean "the trainer's own stream" to oaz_trainer_set_stream and
    # leave the all-reduce unordered against backward / apply)
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        out = _epochs_dp(trainer, attach, n_samples, epochs, batch, seed, rank, world, comm, shard, ts.cuda_stream,
                         reflect, subset)
    trainer.sync()
    trainer.set_stream(None)
    return out


def _epochs_dp(trainer, attach, n_samples, epochs, batch, seed, rank, world, comm, shard, stream,
               reflect=0, subset=None) -> List[EpochLoss]:
    """attach(): makes the n_samples records the trainer's (load_samples or bind_device_samples)."""
    import torch
    subset, n_samples = _subset(subset, n_samples)
    trainer.set_stream(stream)
    dev = f"cuda:{torch.cuda.current_device()}"
    ptr, n = trainer.grads_device()
    grads = torch.as_tensor(_DeviceArray(ptr, n), device=dev)
    nbn = int(trainer._lib.oaz_trainer_bn_stats_count(trainer.blocks))
    bn = torch.empty(nbn, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(seed)
    flag_rng = np.random.default_rng([REFLECT_TAG, seed])
    attach()
    out: List[EpochLoss] = []
    for _ in range(epochs):
        if n_samples < batch:
            break
        idx, flags = epoch_batches(rng, flag_rng, n_samples, batch, reflect, rank, world, subset)
        nb = len(idx)
        assert idx.shape[1] == shard
        _set_batches(trainer, idx, flags)
        for b in range(nb):
            trainer.backward(b)
            if world > 1:
                _allreduce_sum(grads, comm, stream)
            trainer.apply(1.0 / world)
        v, p, k = trainer.losses()
        if world > 1:
            trainer._check(trainer._lib.oaz_trainer_bn_stats_pack(trainer._h, C.c_void_p(bn.data_ptr())))
            _allreduce_sum(bn, comm, stream)
            trainer._check(trainer._lib.oaz_trainer_bn_stats_unpack(trainer._h, C.c_void_p(bn.data_ptr()),
                                                                    C.c_float(1.0 / world)))
            tot = torch.tensor([v, p], dtype=torch.float32, device=dev)
            _allreduce_sum(tot, comm, stream)
            torch.cuda.current_stream().synchronize()
            v, p = (float(x) / world for x in tot.tolist())
        out.append(EpochLoss((v + p) / k, v / k, p / k, k))
    return out
