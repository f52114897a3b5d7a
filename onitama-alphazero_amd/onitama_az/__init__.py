"""onitama_az — MI355X-native Onitama AlphaZero self-play engine (host-side Python mirror).

The compute path is libonitama_az.so (HIP kernels for gfx950 behind the C ABI in
include/onitama_az.h). This package mirrors the reference's Python-visible names over that
ABI: game.* (onitama-game), mcts.* / selfplay.* (alphazero-training).
"""
from . import _abi
from ._abi import OazError, load
from .engine import Engine, SearchResult
from .game import (CARD_NAMES, ORIGINAL_CARDS, Card, Deck, DoneMove, GameState, Move, MoveResult,
                   PieceKind, PlayerColor, State, reflect_card, reflect_moves, reflect_samples, reflect_square,
                   reflect_states)
from .mcts import (AlphaZeroMcts, AlphaZeroMctsConfig, ConvResNet, ConvResNetConfig, Options,
                   TrainingAlphaZeroMcts, reward)
from .selfplay import SelfPlayData, TrainConfig, self_play
from .evaluator import (AlphaZeroAgent, EloRating, Evaluator, EvaluatorConfig, FightStatistics, PitStatistics,
                        RandomAgent, fight)
from .arena import NativeRandomAgent, native_fight
from .pure_mcts import Mcts, pure_mcts_search, pure_mcts_search_each
from .alpha_beta import AlphaBeta, alpha_beta_generate_move, alpha_beta_search
from .tournament import Tournament
from .parameter_check import ParameterCheck
from .replay import ReplayBuffer
from .trainer import (Trainer, choose_batches_doubled, choose_reflect, train_epochs, train_epochs_device,
                      train_epochs_dp, train_epochs_dp_device)
from .train_loop import LoopConfig, Stats, train

__all__ = [
    "_abi", "OazError", "load", "Engine", "SearchResult", "CARD_NAMES", "ORIGINAL_CARDS", "Card", "Deck",
    "DoneMove", "GameState", "Move", "MoveResult", "PieceKind", "PlayerColor", "State", "AlphaZeroMcts",
    "AlphaZeroMctsConfig", "ConvResNet", "ConvResNetConfig", "Options", "TrainingAlphaZeroMcts", "reward",
    "SelfPlayData", "TrainConfig", "self_play", "AlphaZeroAgent", "EloRating", "Evaluator", "EvaluatorConfig",
    "FightStatistics", "PitStatistics", "RandomAgent", "fight", "Mcts", "pure_mcts_search", "Trainer", "train_epochs",
    "LoopConfig", "Stats", "train", "AlphaBeta", "alpha_beta_search", "NativeRandomAgent", "native_fight",
    "alpha_beta_generate_move", "Tournament", "pure_mcts_search_each", "ParameterCheck",
    "reflect_square", "reflect_card", "reflect_states", "reflect_moves", "reflect_samples", "choose_reflect",
    "choose_batches_doubled", "train_epochs_dp", "ReplayBuffer", "train_epochs_device", "train_epochs_dp_device",
]
