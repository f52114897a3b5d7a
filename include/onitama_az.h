/*
 * onitama_az.h — C ABI of the MI355X-native Onitama AlphaZero self-play engine.
 *
 * This is the drop-in boundary for the reference's hot path (cyoq/onitama-alphazero):
 * batched 5x5-bitboard move generation / state stepping (onitama-game) plus
 * leaf-evaluated AlphaZero MCTS (select/expand/backup) and the ResNet policy-value
 * evaluation (alphazero-training). The reference is Rust calling libtorch through
 * tch-rs; a Rust host binds this header with one `extern "C"` block
 * and tch is no longer needed on the path.
 *
 * Conventions
 *   - Plain C, POD structs, caller-owned buffers, no torch types.
 *   - Every function returning int: 0 = OK, < 0 = error; the message is then in
 *     oaz_last_error() (thread-local). Nothing throws or aborts across the ABI:
 *     the reference's panics (e.g. "Must find the best child",
 *     alphazero-training/src/alphazero_mcts/mcts_arena.rs:94,220) become defined
 *     behaviour or an error code.
 *   - An engine is owned by one host thread and bound to one GPU (one process per
 *     GPU, one engine per process in the self-play bench). Distinct engines are
 *     independent, also when several threads create and drive engines on one GPU at
 *     once (creation zeroes and uploads on the engine's own stream and waits for it).
 *   - Engine, trainer and communicator calls run on their object's device and restore
 *     the calling thread's current HIP device before returning (so do the pure-MCTS and
 *     alpha-beta searches on cfg->device); the stateless rules entry points (oaz_movegen, oaz_step,
 *     oaz_current_state, oaz_encode) run on the thread's current device.
 *   - Compute entry points need a gfx950 GPU. Without one oaz_create() returns
 *     NULL and the rules entry points return OAZ_ERR_NO_DEVICE; there is no CPU
 *     fallback in this library.
 *
 * Reference interfaces replaced (file:line under the reference root):
 *   oaz_movegen        <- State::generate_all_legal_moves   onitama-game/src/game/state.rs:301-378
 *   oaz_step           <- State::make_move + Deck::rotate    onitama-game/src/game/state.rs:145-202, deck.rs:87-90
 *   oaz_current_state  <- State::current_state               onitama-game/src/game/state.rs:120-134
 *   oaz_encode         <- create_tensor_from_state           alphazero-training/src/common.rs:26-80
 *   oaz_nn_forward     <- ConvResNet::forward(train=false)   alphazero-training/src/net.rs:215-232
 *   oaz_search         <- MctsArena::new + search            alphazero-training/src/alphazero_mcts/mcts_arena.rs:48-124
 *                         (TrainingAlphaZeroMcts::generate_move_tensor, alphazero_mcts/mod.rs:63-78,
 *                          and Agent::generate_move for AlphaZeroMcts, alphazero_mcts/mod.rs:122-144)
 *   oaz_selfplay_*     <- self_play                           alphazero-training/src/train.rs:35-98
 *   oaz_load_weights   <- AlphaZeroMcts::from_model_file      alphazero-training/src/alphazero_mcts/mod.rs:89-105
 *   oaz_pure_mcts_*    <- Mcts agent (random-rollout UCT)     onitama-game/src/ai/mcts/mcts_arena.rs:56-264, mod.rs:37-52
 *   oaz_alphabeta_*    <- AlphaBeta agent + Evaluation         onitama-game/src/ai/alpha_beta/mod.rs:35-183, evaluation.rs:24-110
 *   oaz_trainer_*      <- the training loop body               alphazero-training/src/train.rs:264-313
 *                         (ConvResNet::forward(train=true) net.rs:215-232, alphaloss net.rs:234-243,
 *                          nn::Sgd{momentum 0.9} + set_weight_decay train.rs:181-186, opt.backward_step)
 */
#ifndef ONITAMA_AZ_H
#define ONITAMA_AZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OAZ_ABI_VERSION 5

/* ---- enums mirroring the reference --------------------------------------- */
enum { OAZ_RED = 0, OAZ_BLUE = 1 };                 /* PlayerColor, player_color.rs:7-10 */
enum { OAZ_PAWN = 0, OAZ_KING = 1 };                /* PieceKind, piece.rs:5-9 */
enum {                                              /* MoveResult, move_result.rs:4-9 */
    OAZ_CAPTURE = 0,
    OAZ_RED_WIN = 1,
    OAZ_BLUE_WIN = 2,
    OAZ_IN_PROGRESS = 3
};
/* Card ids are indices into ORIGINAL_CARDS (card.rs:465-468):
 * 0 Tiger 1 Dragon 2 Frog 3 Rabbit 4 Crab 5 Elephant 6 Goose 7 Rooster
 * 8 Monkey 9 Mantis 10 Crane 11 Horse 12 Ox 13 Boar 14 Eel 15 Cobra. */
enum { OAZ_NUM_CARDS = 16, OAZ_MAX_MOVES = 40 };    /* 2 cards x 5 pieces x 4 squares */

enum {
    OAZ_OK = 0,
    OAZ_ERR_ARG = -1,
    OAZ_ERR_NO_DEVICE = -2,
    OAZ_ERR_HIP = -3,
    OAZ_ERR_CAPACITY = -4,
    OAZ_ERR_STATE = -5,
    OAZ_ERR_WEIGHTS = -6,
    OAZ_ERR_RANGE = -7,     /* ABI 1 only: ABI 2 recomputes fp16-range tiles instead (oaz_nn_fallbacks) */
    OAZ_ERR_COMM = -8,      /* RCCL communicator error (oaz_comm_*, oaz_allgather_samples) */
    OAZ_ERR_INTERNAL = -9   /* a device-side invariant did not hold (oaz_replay_view: the key table overflowed) */
};

enum { OAZ_EVAL_NN = 0, OAZ_EVAL_HASH = 1 };        /* leaf evaluator (HASH: test evaluator, below) */
/* NN arithmetic. OAZ_FP32: exact fp32 MFMA products (v_mfma_f32_16x16x4_f32). OAZ_BF16: bf16 MFMA
 * inputs, fp32 accumulate (BASELINE C5). OAZ_FP32_SPLIT: fp32 operands split exactly into three
 * bf16 terms (hi + mid + lo), the six products above 2^-24 relative on bf16 MFMA, fp32
 * accumulate: fp32-level error (DESIGN.md "fp32 split") at bf16 MFMA rates. OAZ_FP32_SPLIT16: fp32
 * operands split into two fp16 terms (hi = fp16(x), lo = fp16(x - hi): 22 significant bits), the
 * three products hi*hi, hi*lo, lo*hi on fp16 MFMA, fp32 accumulate; conv weights are pre-scaled per
 * output channel by a power of two (exact). Errors vs a float64 forward are at the fp32 level
 * (DESIGN.md "fp16 split") at half the MFMA work of OAZ_FP32_SPLIT. fp16 terms cover |x| < 65504:
 * a workgroup whose 16 positions split an activation beyond that recomputes them in the same launch
 * with the OAZ_FP32_SPLIT arithmetic (fp32 range), so no result is ever silently wrong and no run
 * fails; oaz_nn_fallbacks() counts the recomputed 16-position tiles. */
enum { OAZ_FP32 = 0, OAZ_BF16 = 1, OAZ_FP32_SPLIT = 2, OAZ_FP32_SPLIT16 = 3 };

/* ---- PODs ----------------------------------------------------------------- */

/* State (state.rs:51-56) plus the side to move (MctsState.player_color, mcts_arena.rs:24-28).
 * Bitboards: square i = row*5+col, (0,0) = a5 top-left, bit for square i is 1u<<(31-i)
 * (common/mod.rs:2-16). cards[] are deck slots R0,R1,B2,B3,N4 (deck.rs:14-18). */
typedef struct oaz_state {
    uint32_t kings[2];
    uint32_t pawns[2];
    uint8_t cards[5];
    uint8_t to_move;
    uint8_t pad[2];
} oaz_state; /* 24 bytes */

/* DoneMove (done_move.rs:3-7): Move{from,to,piece} (move.rs:20-25) + used_card_idx (deck slot). */
typedef struct oaz_move {
    uint8_t from;
    uint8_t to;
    uint8_t piece;
    uint8_t slot;
} oaz_move;

/* One MCTS node as stored on the GPU (MctsNode, mcts_arena.rs:355-373). Children of a node
 * are contiguous: [first, first+nch). Node indices are the reference arena indices
 * (allocation order), so a dump compares index-for-index with the reference tree. */
typedef struct oaz_node {
    double W;        /* reward sum ("reward") */
    double P;        /* prior ("probability") */
    uint32_t N;      /* visits */
    uint32_t first;  /* first child (valid when expanded) */
    uint16_t mv;     /* packed move: from | to<<5 | slot<<10 | piece<<12 */
    uint8_t nch;     /* number of children */
    uint8_t flags;   /* bit0 expanded, bit1 terminal */
    uint32_t pad;    /* 0. The leaf-parallel search (oaz_config.leaf_batch) keeps a node's in-flight count here
                      * during a round and leaves 0 after every round. With tree reuse the re-rooting kernel uses this word as its scratch while it runs and
                      * leaves 0 again in every node; only a tree dumped after that kernel was cut short (a
                      * failed launch, a reset device) can show other values here */
} oaz_node; /* 32 bytes */

/* Self-play training sample (SelfPlayData, train.rs:27-33): encoded compactly; the 21x5x5
 * planes are recoverable with oaz_encode(state). */
typedef struct oaz_sample {
    oaz_state state;  /* position before the move; state.to_move = player_color */
    float pi[50];     /* visit distribution [2][25] (calculate_priors, mcts_arena.rs:104-124) */
    float z;          /* reward(final result, player_color) (train.rs:83-85) */
} oaz_sample; /* 228 bytes */

typedef struct oaz_config {
    int32_t blocks;          /* ConvResNetConfig.resnet_block_amnt (net.rs:74-89) */
    int32_t channels;        /* hidden_channels: 64 (only value supported) */
    int32_t in_planes;       /* input_channels: 21 (only value supported) */
    int32_t sims;            /* AlphaZeroMctsConfig.max_playouts; search_time is not used */
    double c_puct;           /* exploration_c */
    int32_t train_noise;     /* AlphaZeroMctsConfig.train: Dirichlet noise at the root */
    int32_t max_plies;       /* TrainConfig.max_plies (train.rs:52,74-79): 150 => 152 plies */
    double dirichlet_alpha;  /* 0.03 (mcts_arena.rs:187) */
    double dirichlet_eps;    /* 0.25 (mcts_arena.rs:186) */
    int32_t games;           /* parallel game slots G (also the max batch of oaz_search) */
    int32_t evaluator;       /* OAZ_EVAL_NN or OAZ_EVAL_HASH */
    int32_t precision;       /* OAZ_FP32, OAZ_BF16, OAZ_FP32_SPLIT or OAZ_FP32_SPLIT16 (default) */
    int32_t fixed_deck;      /* 1: every game uses deck[]; 0: random 5 of 16 per game (deck.rs:139-151) */
    uint8_t deck[5];
    uint8_t temperature_plies; /* self-play temperature (DESIGN.md "Self-play temperature"): 0 = off (default, and
                                what a zeroed pad byte of an older caller means): every ply plays the most
                                visited move. T > 0: in a game's first T plies (ply < T) the played move is drawn
                                in proportion to the root children's visits (tau = 1, exact in integers, keyed
                                by seed, game id and ply: oaz_temperature_pick); later plies play the most
                                visited move. The recorded pi is the visit distribution either way. Self-play
                                only: oaz_search, the arena and the Agent API ignore it */
    uint8_t leaf_batch;      /* leaf-parallel search (DESIGN.md "Leaf-parallel search"): 0 = off (default, and what a
                                zeroed pad byte of an older caller means): the searches, memory and launches of an
                                engine without the feature. L = 1 .. 16: oaz_search and the arena's resident search
                                of at most CU-count roots collect up to L leaves of a root's tree per network pass
                                (virtual loss: every node has an in-flight count, oaz_node.pad, 0 outside a round)
                                and evaluate them as one 16-position tile, one launch for the whole search. L = 1
                                is the sequential search bit for bit; from L + 1 playouts on the trees differ from
                                it, by the rule stated in DESIGN.md. Needs step_kernels = 0, compact = 0,
                                reuse_visits = 0 and the fp16x3 network or HASH (checked at creation); a search
                                with root noise or more roots than CUs, and self-play, fail with OAZ_ERR_STATE:
                                there is no fallback to another algorithm. Values above 16 are rejected */
    uint8_t pad0[1];
    uint64_t seed;           /* counter-based RNG key for deals, Dirichlet noise and temperature draws */
    int32_t rank;            /* global game id = (k * world + rank) * games + slot */
    int32_t world;
    int32_t sample_capacity; /* max samples buffered on the device (0: auto) */
    int32_t stagger;         /* self-play: slot g starts playing after g % stagger plies (steady-state
                                game ages for throughput measurement); 0 = all slots start at once */
    int32_t compact;         /* leaf compaction: only the leaves whose evaluation the playout uses go to
                                the evaluator (a won, terminal-flagged leaf's is computed and discarded by
                                the reference, Q2). 0 = off: every playout evaluates its leaf, as the
                                reference (default); 1 = always; 2 = when it saves NN workgroup rounds
                                (games >= 12 * 16 * CUs). Trees, pi and samples are identical either way */
    int32_t parts;           /* the simulation loop runs the games in this many parts (1, 2 or 4), each
                                on its own stream so one part's tree kernels fill the others' NN gaps;
                                0 = auto (2 from 2048 games); results are identical either way */
    int64_t search_time_ns;  /* Q7, AlphaZeroMctsConfig.search_time (mcts_arena.rs:78: playouts run while
                                `playouts < max_playouts && elapsed < search_time`). 0 = off (default, the
                                parity mode: exactly `sims` playouts). > 0: a search (or self-play ply) stops
                                after the first simulation step that ends at or past this wall-clock budget
                                from its start, and pi / the move come from the visits that ran. A search
                                of the one-launch sizes (step_kernels 0: <= CU-count games without root
                                noise, or <= 16 x CU-count games) reads the device clock before every
                                simulation, each game (k_search_grp: each 16-game group) on its own, so the
                                games of a batch may run different counts (>= 1, <= sims;
                                oaz_search_playouts); larger batches stop together after a simulation step */
    int32_t step_kernels;    /* 0 = auto: a search of at most CU-count games with the fp16x3 network (or
                                HASH), no root noise and no leaf compaction runs as ONE
                                launch, a workgroup per game doing all its simulations (the Agent API's
                                one-position latency path); 1 = always the per-simulation-step launches.
                                Trees, pi and samples are identical either way */
    int32_t reuse_visits;    /* tree reuse (DESIGN.md "Tree reuse"): 0 = off (default): a fresh tree per search
                                and per self-play ply, the memory and behaviour of an engine without the
                                feature. R > 0 (R >= sims): a tree's capacity in root visits; trees hold
                                1 + R * OAZ_MAX_MOVES nodes (device memory for trees grows by R / sims). A
                                self-play ply, and oaz_search_advance, then keep the played move's subtree for
                                the next search when the moved-to child is expanded, not terminal-flagged, the
                                move does not win, and the child's visits + the creation `sims` <= R; the next
                                search adds `sims` playouts to the kept ones */
} oaz_config;

typedef struct oaz_search_stats {
    uint64_t sims;            /* simulations run (= NN leaf evaluations, Q2) */
    uint64_t expansions;      /* leaves actually expanded (non-terminal, first visit) */
    uint64_t children;        /* children created */
    uint64_t terminal_leaves; /* playouts that ended on a won position */
    uint64_t depth_sum;       /* sum of select path depths */
    uint64_t stuck_leaves;    /* expanded nodes with no legal move (reference panics, Q6) */
    uint64_t max_nodes;       /* largest tree seen */
    uint64_t nn_evals;        /* leaf evaluations whose policy or value the playout uses: every
                               * playout except those ending on a won, already terminal-flagged
                               * node, whose evaluation the reference computes and then discards
                               * (mcts_arena.rs:156-176); only these are sent to the network */
} oaz_search_stats;

typedef struct oaz_selfplay_stats {
    uint64_t moves;           /* plies played over all slots */
    uint64_t games_finished;
    uint64_t games_cut;       /* finished by the ply cap (z = 0) */
    uint64_t red_wins, blue_wins;
    uint64_t samples_ready;   /* samples buffered on the device */
    uint64_t samples_dropped; /* overflowed the device buffer */
    uint64_t passes;          /* root positions with no legal move: pass (Q6) */
    oaz_search_stats search;
} oaz_selfplay_stats;

typedef struct oaz_kernel_times {
    /* accumulated HIP-event time (ms) and launches per kernel class; enabled with
     * oaz_set_timing(eng, 1) */
    double select_ms, nn_ms, expand_ms, finalize_ms;
    uint64_t select_n, nn_n, expand_n, finalize_n;
    uint64_t nn_samples;  /* positions of the timed nn launches outside the simulation loop (oaz_nn_forward,
                           * root values); in the loop the count is on the device: oaz_search_stats.nn_evals */
    double noise_ms;      /* Dirichlet root-noise producer (second stream, overlaps the NN) */
    uint64_t noise_n;
    double compact_ms;    /* leaf compaction (the positions the NN evaluates, per 4096-game bucket) */
    uint64_t compact_n;
    double backup_select_ms; /* expand/backup of simulation s fused with the select of s + 1 (every
                              * simulation step but the first select and the last expand/backup) */
    uint64_t backup_select_n;
    double nn_busy_ms;    /* length of the union of the timed nn launches' intervals (the game parts'
                           * launches of one simulation step overlap; oaz_config.parts) */
    uint64_t nn_busy_n;   /* disjoint intervals in that union */
    uint64_t parts;       /* game parts (streams) of the last simulation loop: nn launches per step */
} oaz_kernel_times;

typedef struct oaz_engine oaz_engine;

/* ---- library ---------------------------------------------------------------- */
int oaz_abi_version(void);
const char* oaz_last_error(void);
void oaz_config_default(oaz_config* cfg);   /* canonical self-play config (bin/train.rs:50-78) */
int oaz_device_count(int* n);               /* number of visible HIP devices */

/* ---- host-side helpers (no GPU needed) ---------------------------------------- */
/* ATTACK_MAPS[color][card][from] (card.rs:476-604), as compiled into the kernels. */
void oaz_attack_maps(uint32_t out[2 * 16 * 25]);
/* Number of fp32 values in the canonical weight blob (tch VarStore order). */
size_t oaz_weight_count(int blocks, int channels, int in_planes);
/* Bytes of the packed, BN-folded weight image the network kernels read for `precision` (OAZ_FP32 ...
 * OAZ_FP32_SPLIT16): every launch streams it into each XCD's L2 once (the L2s are written back and
 * invalidated at kernel boundaries), which is the per-launch weight traffic bench.py's roofline counts. */
size_t oaz_nn_device_bytes(int blocks, int precision);
/* Random-init weights in canonical order: conv/linear U(-1/sqrt(fan_in), +1/sqrt(fan_in)),
 * BN gamma 1, beta 0, mean 0, var 1. */
int oaz_random_weights(uint64_t seed, int blocks, float* out, size_t n);
/* Deck of global game `game_id` under `seed` (random 5 of 16, Fisher-Yates on Philox). */
void oaz_deal_deck(uint64_t seed, uint64_t game_id, uint8_t out[5]);
/* Global game ids of the `games` self-play slots of rank `rank` of `world` in their seq-th game:
 * out[g] = (seq * world + rank) * games + g, the rule the self-play kernel keys deals and root noise with
 * (replaces the reference's per-worker games, train.rs:218-238: ranks play disjoint game ids). */
int oaz_slot_game_ids(int rank, int world, int games, uint64_t seq, uint64_t* out);
/* Start position with `deck`; to_move = colour of the neutral card (game_state.rs:19-24). */
void oaz_initial_state(const uint8_t deck[5], oaz_state* out);
/* The HASH test evaluator (identical on host and device; documented in DESIGN.md). */
void oaz_hash_eval(const oaz_state* s, float policy[50], float* value);
/* One root-noise draw (replaces the per-comparison Dirichlet(alpha; K) sample of
 * mcts_arena.rs:186-203, marginally Beta(alpha, (K-1) alpha), f64 as the reference's): draw `draw`
 * (2j + 0 for the running best, 2j + 1 for child j of comparison j) of simulation `sim` at ply `ply`
 * of global game `game_id`. Host computation of the exact value the GPU's root-noise kernel stores. */
double oaz_root_noise(uint64_t seed, uint64_t game_id, uint32_t ply, uint32_t sim, uint32_t draw, double alpha,
                      int nchild);
/* The self-play temperature rule (oaz_config.temperature_plies), restated on the host; needs no device. The root's
 * children j = 0 .. K-1 in node order have visits[j], S = their sum (uint32; a tree's fits). With w = word 0 of
 * Philox(seed; game_id lo, game_id hi, 0x54454D50, ply) and r = (w * S) >> 32, the played child is the first j
 * whose inclusive prefix sum visits[0] + .. + visits[j] exceeds r. Returns that child; -1 when the rule draws
 * nothing (K <= 0, null visits or S == 0: the pass or the most visited child is played, as without temperature).
 * T does not enter: whether ply < T is the caller's question. */
int oaz_temperature_pick(uint64_t seed, uint64_t game_id, uint32_t ply, const uint32_t* visits, int K);
/* The playout cap rule (oaz_selfplay_set_playout_cap), restated on the host; needs no device. Ply `ply` of global
 * game `game_id` is a full ply iff word 0 of Philox(seed; game_id lo, game_id hi, 0x50434150, ply), shifted right by
 * 16, is below full_per_65536. Returns 1 (full) or 0 (fast); OAZ_ERR_ARG for full_per_65536 > 65536. */
int oaz_playout_cap_full(uint64_t seed, uint64_t game_id, uint32_t ply, uint32_t full_per_65536);

/* ---- rules on the GPU (bit-exact with the reference) ---------------------------- */
/* Legal moves of s[i].to_move. masks[i][k][from] = destination mask of own piece on
 * `from` with the mover's k-th card (slot 0/1 for Red, 2/3 for Blue), 0 if no own piece.
 * moves[i][*] in reference order (slot, from, to ascending), the entries past counts[i] zero;
 * counts[i] = #moves.
 * Any output pointer may be NULL. Host pointers. */
int oaz_movegen(const oaz_state* s, int n, uint32_t* masks /* n*2*25 */,
                oaz_move* moves /* n*40 */, uint8_t* counts /* n */);
/* make_move(mv[i], s[i].to_move, mv[i].slot) in place, then switch to_move;
 * results[i] = MoveResult. Host pointers. */
int oaz_step(oaz_state* s, const oaz_move* mv, int n, uint8_t* results);
/* current_state() of each position. */
int oaz_current_state(const oaz_state* s, int n, uint8_t* results);
/* 21x5x5 planes of s[i] for colour s[i].to_move (fp32, n*525). */
int oaz_encode(const oaz_state* s, int n, float* planes);

/* ---- engine --------------------------------------------------------------------- */
oaz_engine* oaz_create(const oaz_config* cfg, int device);
void oaz_destroy(oaz_engine* eng);
int oaz_get_config(const oaz_engine* eng, oaz_config* out);
/* Per-agent search parameters for the following searches / self-play plies (AlphaZeroMctsConfig,
 * alphazero_mcts/mod.rs:26-43: max_playouts <= the creation cfg.sims, exploration_c, train), so
 * agents with different configs can share one engine as the reference's agents share one
 * Arc<Mutex<ConvResNet>> (mod.rs:84,124). */
int oaz_set_search_params(oaz_engine* eng, int sims, double c_puct, int train_noise);
/* Q7 wall-clock budget per search (AlphaZeroMctsConfig.search_time, alphazero_mcts/mod.rs:26-43;
 * the reference's default agent: 400 ms / 5000 playouts, its tournament: 1 s / 5000,
 * bin/tournament.rs:121-129) for the following searches / plies: oaz_config.search_time_ns. 0 = off. */
int oaz_set_search_time(oaz_engine* eng, int64_t search_time_ns);
/* Simulations per game run by the last search / self-play ply (= sims unless a search_time_ns budget
 * stopped it earlier; with per-game counts, their maximum). */
int oaz_last_sims(oaz_engine* eng, int* sims);
/* Playouts each of the first G games of the last search / ply ran (the reference's
 * MctsArena.playouts after search(), mcts_arena.rs:75-81); G <= the last call's games. */
int oaz_search_playouts(oaz_engine* eng, int* out, int G);
/* Leaf-parallel search (oaz_config.leaf_batch > 0): out[0] = rounds (network passes), out[1] = playouts and
 * out[2] = discarded walks (a walk that reached a leaf already in flight closes its round and counts no playout)
 * of the last search, summed over its roots. All 0 with leaf_batch == 0 or before the first search. */
int oaz_search_leaf_batch_stats(oaz_engine* eng, uint64_t out[3]);
/* Weights in canonical order (n == oaz_weight_count). BN is folded on the host. */
int oaz_load_weights(oaz_engine* eng, const float* blob, size_t n);

/* ---- model loading by name (AlphaZeroMcts::from_model_file: `vs.load(model_path)` on the
 * ConvResNet of net.rs:101-213, alphazero_mcts/mod.rs:89-105) ----------------------------------
 * The canonical tensor table = the VarStore variables net.rs creates, in creation order (the blob
 * layout of oaz_load_weights): names joined with '|' as in the .ot files ('.' — tch's in-memory
 * separator — is accepted everywhere a name is taken). Host-only helpers (no GPU). */
size_t oaz_weight_tensor_count(int blocks);
int oaz_weight_tensor_info(int blocks, size_t i, char* name, size_t name_cap, size_t* numel);
/* n named fp32 tensors (any order, e.g. tch's `vs.variables()` HashMap: name, data pointer, numel)
 * -> the canonical blob (out_n >= oaz_weight_count). A missing, duplicate, unknown or wrongly sized
 * tensor is OAZ_ERR_WEIGHTS naming it (the reference silently keeps random weights, Q13). */
int oaz_weights_from_named(int blocks, const char* const* names, const float* const* data, const size_t* sizes,
                           size_t n, float* out, size_t out_n);
/* The same, straight into an engine (blocks = the engine's). */
int oaz_load_weights_named(oaz_engine* eng, const char* const* names, const float* const* data,
                           const size_t* sizes, size_t n);
/* A VarStore::save .ot archive (train.rs:414-430; TorchScript zip with stored members) -> canonical
 * blob; *blocks_out = residual blocks found in it. data.pkl is read by a restricted pickle machine
 * that builds plain values only (nothing is imported or executed). out may be NULL to size. */
int oaz_ot_read(const char* path, float* out, size_t cap, size_t* n_out, int* blocks_out);
/* oaz_ot_read + oaz_load_weights; the file must hold a network of the engine's block count. */
int oaz_load_ot(oaz_engine* eng, const char* path);
/* ---- checkpoints (save_vs, alphazero-training/src/train.rs:414-430: `vs.save(&path)`) ---------
 * A canonical blob (n == oaz_weight_count(blocks, 64, 21)) -> a VarStore .ot archive at `path`: the
 * TorchScript zip layout VarStore::load, oaz_ot_read and torch.jit.load read (stored members under
 * "<file stem>/", '|' names, 64-byte aligned fp32 storages). Written to "<path>.tmp" and renamed
 * over `path`. Host only. */
int oaz_ot_write(const char* path, const float* blob, size_t n, int blocks);
/* save_vs naming: "<folder>/[best_]model_<iteration>_<stamp>.ot", stamp NULL = the local time as
 * "%Y%m%d_%H%M%S" (chrono Local::now()). OAZ_ERR_CAPACITY if out[cap] is too small. */
int oaz_checkpoint_path(const char* folder, int64_t iteration, int is_best, const char* stamp, char* out,
                        size_t cap);
int oaz_sync(oaz_engine* eng);
/* enable: 0 off, 1 HIP events around every launch, N > 1 around the kernels of every N-th
 * simulation step only (the events cost ~2 % of a C3 step when every launch is timed). */
int oaz_set_timing(oaz_engine* eng, int enable);
int oaz_kernel_times_get(oaz_engine* eng, oaz_kernel_times* out);
int oaz_kernel_times_reset(oaz_engine* eng);

/* policy [B][2][25] (softmax over all 50), value [B]. Host pointers. B <= cfg.games. */
int oaz_nn_forward(oaz_engine* eng, const oaz_state* s, int B, float* policy, float* value);
/* OAZ_FP32_SPLIT16: 16-position tiles recomputed with the OAZ_FP32_SPLIT arithmetic because an
 * activation left the fp16 range, since the engine was created (0 for other precisions). */
int oaz_nn_fallbacks(oaz_engine* eng, uint64_t* tiles);

/* One search per root (root colour = roots[i].to_move), cfg.sims simulations each, all
 * G searches advanced together. out_pi [G][50] f32, out_root_value [G] = an extra NN
 * evaluation of the root (Agent::generate_move, mod.rs:137-141). Any output may be NULL. */
int oaz_search(oaz_engine* eng, const oaz_state* roots, int G, oaz_move* out_move,
               float* out_pi, float* out_root_value, oaz_search_stats* stats);
/* Tree of `game` left by the last oaz_search, or of slot `game` by the last self-play ply (the tree that
 * ply's move and pi came from): nodes [0, *n_nodes) in reference arena order. */
int oaz_tree_dump(oaz_engine* eng, int game, oaz_node* out, int cap, int* n_nodes);

/* ---- tree reuse (oaz_config.reuse_visits > 0; DESIGN.md "Tree reuse") -------------------------
 * The subtree of a root child c, taken out of a search tree with its node order kept, equals node for node
 * the tree of a fresh search from c's position with N_c playouts (HASH evaluator, no root noise), so a
 * search resumed on it for `sims` more playouts equals a fresh search of N_c + sims playouts. */
typedef struct oaz_reuse_stats {
    uint64_t trees_kept;   /* searches (self-play plies of playing slots, advanced games) that began on a kept subtree */
    uint64_t trees_fresh;  /* ... and on a fresh tree (game starts, passes, the keep rule said no) */
    uint64_t visits_kept;  /* sum of the kept children's N: playouts those searches did not have to redo */
    uint64_t nodes_kept;   /* sum of the kept subtrees' node counts */
} oaz_reuse_stats;
/* Re-roots the first G trees of the last oaz_search / oaz_search_resume at moves[g] and steps the engine's
 * resident root positions by them (the side to move flips). Where the keep rule holds (oaz_config.reuse_visits)
 * the moved-to child's subtree becomes the tree and kept[g] (optional, [G]) is that child's N; otherwise the
 * game gets a fresh tree and kept[g] = 0. A pass (from = to = 25, slot = one of the mover's cards, which goes
 * round with the neutral card) is accepted only at a root without a child and leaves a fresh tree.
 * OAZ_ERR_STATE: reuse_visits == 0, the last search covered fewer than G games, or self-play or an arena fight
 * on this engine ran in between.
 * OAZ_ERR_ARG: a move that is neither a child of its root nor an accepted pass; the moves are validated by a
 * kernel that changes nothing, so on this error no tree and no root has changed for any game. */
int oaz_search_advance(oaz_engine* eng, const oaz_move* moves, int G, int32_t* kept);
/* oaz_search on the engine's resident roots (the positions oaz_search_advance stepped to; out_roots,
 * optional [G], receives them) without the tree reset: cfg.sims more playouts per game on the trees as
 * they are, by the per-simulation-step kernels. Outputs as oaz_search's. OAZ_ERR_STATE: reuse_visits == 0,
 * no search of at least G games came before, or the trees cannot hold sims more playouts (a second resume
 * without an advance in between, past reuse_visits root visits). */
int oaz_search_resume(oaz_engine* eng, int G, oaz_move* out_move, float* out_pi, float* out_root_value,
                      oaz_search_stats* stats, oaz_state* out_roots);
/* The counters since creation or the last oaz_selfplay_reset (all 0 with reuse_visits == 0). */
int oaz_reuse_stats_get(oaz_engine* eng, oaz_reuse_stats* out);
/* The re-rooting the device does, restated on the host (host only; the compaction is stated once, in
 * csrc/oaz_tree_rebase.h, for both): in[0, n) is a tree as oaz_tree_dump gives it, child the index among the
 * root's children (0 .. nch - 1) of a visited child; out[0, *n_out) becomes that child's subtree in the same
 * node order, `first` indices remapped, the new root with P = 1 and mv = 0. OAZ_ERR_ARG for a child the root
 * does not have or one with N == 0, OAZ_ERR_CAPACITY when the subtree exceeds cap; nothing is written then. */
int oaz_tree_rebase_host(const oaz_node* in, int n, int child, oaz_node* out, int cap, int* n_out);
/* After an oaz_search / oaz_search_resume of at least G games: the move the temperature rule draws from game g's
 * resident tree for (game_ids[g], plies[g]) under cfg.seed, for a caller that drives its own game loop (the
 * generate_move_tensor of a sampling agent) and as the direct handle on the device's draw. cfg.temperature_plies
 * does not enter. out_moves [G] and out_child [G] (either may be null): the drawn child's move and its index among
 * the root's children; the most visited child (the last maximum) where no child has a visit; the pass move of
 * oaz_search and child -1 at a root without a child. The trees are not changed.
 * OAZ_ERR_STATE: the last search covered fewer than G games, or self-play or an arena fight ran in between. */
int oaz_search_sample_moves(oaz_engine* eng, int G, const uint64_t* game_ids, const uint32_t* plies,
                            oaz_move* out_moves, int32_t* out_child);

/* ---- self-play (continuous batching over cfg.games slots, device resident) ------ */
int oaz_selfplay_reset(oaz_engine* eng);                 /* deal a fresh game in every slot */
int oaz_selfplay_step(oaz_engine* eng, int moves);       /* play `moves` plies in every slot */
int oaz_selfplay_stats_get(oaz_engine* eng, oaz_selfplay_stats* out);
/* Self-play temperature, since creation or the last oaz_selfplay_reset: out[0] = plies whose move was drawn from
 * the visits, out[1] = those whose drawn child is not the most visited one (both 0 with temperature_plies == 0). */
int oaz_selfplay_temperature_stats(oaz_engine* eng, uint64_t out[2]);
/* Playout cap randomization, an engine setting for the following self-play: a ply that
 * oaz_playout_cap_full(cfg.seed, game id, ply, full_per_65536) calls full is searched with cfg.sims playouts and
 * recorded, every other ply with fast_sims playouts and only played. Both kinds use cfg.c_puct and cfg.train_noise
 * and play the move the engine would play from that tree (the temperature draw, else the last maximum of the visits,
 * the pass at a root without a child). A finished game's records are its full plies in ply order; a game without one
 * gives no record and still counts in games_finished. fast_sims = 0 turns the cap off. Setting or changing the cap
 * ends the running games: the next oaz_selfplay_step starts from a reset, as on a fresh engine. A capped ply runs on
 * the per-simulation-step kernels with leaf compaction on, whatever cfg.compact and cfg.step_kernels say, so that
 * the games that stopped leave the network's batch. The cap's device buffers (7 bytes per slot) are allocated by
 * the first call that sets one. oaz_search, oaz_search_resume, the arena and the agents ignore the cap.
 * OAZ_ERR_ARG: fast_sims < 0, full_per_65536 outside 0 .. 65536, a null engine. OAZ_ERR_STATE (nothing else runs
 * instead): an engine with reuse_visits > 0, leaf_batch > 0 or a search-time budget; and from oaz_selfplay_step
 * while a cap is set and fast_sims >= cfg.sims, or a search-time budget has been set since. */
int oaz_selfplay_set_playout_cap(oaz_engine* eng, int fast_sims, int full_per_65536);
/* out[0] = full plies, out[1] = fast plies played since the last reset (both 0 without a cap);
 * oaz_selfplay_stats.search.sims is then out[0] * cfg.sims + out[1] * fast_sims. */
int oaz_selfplay_playout_cap_stats(oaz_engine* eng, uint64_t out[2]);
/* Copy up to cap buffered samples to host memory and drop them from the device buffer. */
int oaz_samples_fetch(oaz_engine* eng, oaz_sample* out, size_t cap, size_t* n_out);
/* Device-to-device copy of up to cap_bytes/sizeof(oaz_sample) buffered samples into a
 * device buffer on the engine's GPU (e.g. a tensor that is then all-gathered over RCCL). */
int oaz_samples_export_device(oaz_engine* eng, void* dev_dst, size_t cap_bytes, size_t* n_out);
/* self_play(): play exactly n_games games and return their samples. n_games counts global game
 * ids over all ranks (cfg.world): this rank plays the ids below n_games that it owns
 * ((k * world + rank) * games + slot) and returns when those are finished. */
int oaz_selfplay_run(oaz_engine* eng, int n_games, oaz_sample* out, size_t cap,
                     size_t* n_out, oaz_selfplay_stats* stats);

/* ---- multi-GPU: RCCL over xGMI ------------------------------
 * One process (or host thread) per GPU, one engine per GPU, games sharded by global game id with
 * no exchange inside the simulation loop. The one data exchange of the path replaces the
 * reference's join of its self-play workers' buffers (alphazero-training/src/train.rs:241-244:
 * `for handle in handles { data_buffer.extend(handle.join()) }`): every rank ends with every
 * rank's (s, pi, z) records. The communicator wraps an RCCL communicator (librccl.so.1, loaded on
 * first use); rank 0 makes the id and the host sends it to the other ranks out of band (a file,
 * a socket, torch.distributed, MPI). All oaz_comm_* calls with a `comm` are collective. */
typedef struct oaz_comm oaz_comm;
typedef struct oaz_comm_id { char internal[128]; } oaz_comm_id;  /* = ncclUniqueId */

int oaz_comm_unique_id(oaz_comm_id* out);
/* Joins `world` ranks on GPU `device`; blocks until all ranks joined. NULL on error. */
oaz_comm* oaz_comm_init(const oaz_comm_id* id, int rank, int world, int device);
void oaz_comm_destroy(oaz_comm* comm);
/* All-gather of the engines' buffered samples: every rank's samples_ready records land in
 * dev_out (device memory on the engine's GPU, cap records) in rank order, and are dropped from each
 * engine's buffer (as oaz_samples_fetch does). counts_out[world] (host, optional) = records per
 * rank; *n_total = their sum. Counts are all-gathered first, then each rank's block is one
 * broadcast into its offset, all in one RCCL group: an all-gatherv with no padding and no scratch.
 * OAZ_ERR_CAPACITY (on every rank alike) when the total exceeds cap; nothing is consumed then. */
int oaz_allgather_samples(oaz_engine* eng, oaz_comm* comm, oaz_sample* dev_out, size_t cap, size_t* n_total,
                          uint64_t* counts_out);
/* In-place sum all-reduce of n floats in device memory (data-parallel gradients), on `stream`
 * (a hipStream_t; NULL = the communicator's own stream); returns when enqueued. */
int oaz_comm_allreduce_sum_f32(oaz_comm* comm, float* dev, size_t n, void* stream);
/* In-place broadcast of `bytes` bytes of device memory from `root` (new best weights),
 * on `stream` (NULL = the communicator's stream); returns when enqueued. */
int oaz_comm_broadcast(oaz_comm* comm, void* dev, size_t bytes, int root, void* stream);
/* Waits for the communicator's own stream. */
int oaz_comm_sync(oaz_comm* comm);
/* What RCCL itself reports for the communicator, and the last oaz_allgather_samples timed by HIP events
 * on the communicator's stream (host copies and any caller-side post-processing excluded). */
typedef struct oaz_comm_stats {
    int32_t ranks;              /* ncclCommCount(): ranks in the RCCL communicator */
    int32_t rank;
    uint64_t allgather_calls;
    double counts_ms;           /* last all-gather: the uint64 counts all-gather (+ its 8-byte host copies) */
    double allgather_ms;        /* last all-gather: the grouped per-rank broadcasts of the 228-byte records */
    uint64_t allgather_records; /* records every rank received in the last all-gather (sum of the counts) */
    uint64_t allgather_bytes;   /* = allgather_records * sizeof(oaz_sample) */
    uint64_t own_records;       /* this rank's contribution to the last all-gather */
} oaz_comm_stats;
int oaz_comm_stats_get(oaz_comm* comm, oaz_comm_stats* out);

/* ---- training step ---------------------------------
 * One trainer = one GPU. Parameters live on the device in the canonical blob
 * layout (the VarStore order, see oaz_weight_count); BN running statistics are
 * part of the blob and are updated by the train-mode forward (momentum 0.1,
 * unbiased variance), as tch's batch_norm2d does. A step is
 *   gather batch -> forward(train=true) -> alphaloss -> backward -> SGD
 * with the reference's optimiser: d = g + wd*p; buf = momentum*buf + d; p -= lr*buf
 * over the trainable variables (weights, biases, BN gamma/beta). */
typedef struct oaz_train_config {
    int32_t blocks;               /* residual blocks (ConvResNetConfig::resnet_block_amnt) */
    int32_t max_batch;            /* largest batch (multiple of 16); train_batch_size 512 (train.rs:142) */
    double learning_rate;         /* 5e-3 (bin/train.rs:69) */
    double momentum;              /* 0.9 (train.rs:182) */
    double weight_decay;          /* l2_const 1e-4 (train.rs:139,186) */
    double bn_momentum;           /* 0.1 (tch BatchNormConfig default) */
    double bn_eps;                /* 1e-5 */
    int32_t value_loss_broadcast; /* 1 = reference (Q16: z[B] - v[B,1] broadcasts to [B,B]), 0 = elementwise */
    int32_t reserved[7];
} oaz_train_config;

typedef struct oaz_trainer oaz_trainer;

void oaz_train_config_default(oaz_train_config* cfg);
oaz_trainer* oaz_trainer_create(const oaz_train_config* cfg, int device);  /* NULL on error */
void oaz_trainer_destroy(oaz_trainer* t);
/* Run the trainer's kernels on `stream` (a hipStream_t; NULL = the trainer's own stream). */
int oaz_trainer_set_stream(oaz_trainer* t, void* stream);
/* Parameters + running stats, canonical blob (n = oaz_weight_count(blocks, 64, 21)).
 * set_weights also clears the momentum buffers (a fresh nn::Sgd). */
int oaz_trainer_set_weights(oaz_trainer* t, const float* blob, size_t n);
int oaz_trainer_get_weights(oaz_trainer* t, float* blob, size_t n);
/* The trainer's parameters (and BN running statistics) as a .ot checkpoint (oaz_ot_write): the
 * reference's save_vs on the training VarStore (train.rs:383-403, 414-430). */
int oaz_trainer_save_ot(oaz_trainer* t, const char* path);
/* The replay buffer: copy n host samples to the device (owned), or bind n samples already
 * resident on this GPU (e.g. oaz_samples_export_device; not owned, must outlive use). */
int oaz_trainer_load_samples(oaz_trainer* t, const oaz_sample* samples, size_t n);
int oaz_trainer_bind_device_samples(oaz_trainer* t, const oaz_sample* dev_samples, size_t n);
/* Upload batch indices (n_batches x batch int32 into the replay buffer), e.g. one epoch of
 * choose_multiple draws (train.rs:272-276). */
int oaz_trainer_set_batches(oaz_trainer* t, const int32_t* idx, int n_batches, int batch);
/* Forward + loss + backward for batch `b` of the uploaded indices: gradients land in the
 * device gradient buffer (oaz_trainer_grads); no parameter changes except BN running stats. */
int oaz_trainer_backward(oaz_trainer* t, int b);
/* Device gradient buffer (canonical blob layout; running-stat slots unused) for an external
 * all-reduce between backward and apply (data-parallel training). */
int oaz_trainer_grads(oaz_trainer* t, float** dev_grads, size_t* n);
int oaz_trainer_get_grads(oaz_trainer* t, float* host, size_t n);
/* SGD step on the gradient buffer (scaled by grad_scale, e.g. 1/world after a sum all-reduce). */
int oaz_trainer_apply(oaz_trainer* t, float grad_scale);
/* BN running statistics (running_mean + running_var of every BN layer, canonical order) as one
 * contiguous device range of oaz_trainer_bn_stats_count(blocks) floats, so a data-parallel host can
 * average them over ranks (pack, oaz_comm_allreduce_sum_f32, unpack with scale = 1/world) and every
 * rank keeps identical inference weights (ranks' batch statistics differ; DDP without SyncBN). Both
 * run on the trainer's stream. */
size_t oaz_trainer_bn_stats_count(int blocks);
int oaz_trainer_bn_stats_pack(oaz_trainer* t, float* dev_out);
int oaz_trainer_bn_stats_unpack(oaz_trainer* t, const float* dev_in, float scale);
/* backward(b) + apply(1) for batches [first, first+count). */
int oaz_trainer_train(oaz_trainer* t, int first, int count);
/* Loss sums since the last call: out[0] value loss, out[1] policy loss, out[2] steps. */
int oaz_trainer_losses(oaz_trainer* t, double out[3]);
int oaz_trainer_sync(oaz_trainer* t);

/* ---- pure MCTS agent --------------------------------
 * The reference's `Mcts` agent: UCT (f32, winrate + c*sqrt(ln N / n)) over a tree expanded once a
 * leaf has more than min_node_visits visits, random rollouts to the end of the game, +-1 backed up
 * with a sign flip. One GPU thread runs one game's whole search. Rollout draws come from Philox
 * (seed; game_id0 + g, playout, 0x9C7A0000, d/4); a rollout longer than rollout_cap plies scores 0. */
typedef struct oaz_pure_mcts_config {
    int32_t max_playouts;     /* 5000 (ai/mcts/mod.rs:25); the arena's opponent uses 400 (evaluator.rs:340-345) */
    int32_t min_node_visits;  /* 5 */
    float exploration_c;      /* sqrt(2) as f32 (the arena's opponent: 1.41) */
    int32_t rollout_cap;      /* plies per rollout before it is scored as a draw (reference: none) */
    uint64_t seed;
    uint64_t game_id0;        /* RNG stream of root g = game_id0 + g */
    int32_t device;           /* HIP device the search runs on (its own stream; other work on it is not waited for) */
    int32_t reserved[3];
} oaz_pure_mcts_config;

typedef struct oaz_pure_node { /* MctsNode (mcts_arena.rs:330-352) */
    uint32_t visits;
    float reward;
    float winrate;
    uint32_t first;   /* first child (children are contiguous) */
    uint32_t parent;  /* 0xFFFFFFFF for the root */
    uint16_t mv;      /* from | to<<5 | slot<<10 | piece<<12 */
    uint8_t nch;
    uint8_t flags;    /* 1 expanded, 2 terminal */
} oaz_pure_node;  /* 24 bytes */

typedef struct oaz_pure_mcts_stats {
    uint64_t playouts, expansions, rollout_plies, rollout_passes, rollouts_capped, max_nodes, tree_full;
} oaz_pure_mcts_stats;

void oaz_pure_mcts_config_default(oaz_pure_mcts_config* cfg);
/* Nodes one search may allocate (the per-game capacity of tree_out). */
size_t oaz_pure_mcts_tree_capacity(const oaz_pure_mcts_config* cfg);
/* One search per root (colour = root.to_move). out_value = winrate of the chosen child. A root with
 * no legal move returns the pass move (from = to = 25). tree_out (optional, G x tree_cap nodes)
 * receives each game's tree. Runs on cfg->device on a stream of its own; the calling thread's current
 * HIP device is restored before the call returns. */
int oaz_pure_mcts_search(const oaz_state* roots, int G, const oaz_pure_mcts_config* cfg, oaz_move* out_move,
                         float* out_value, oaz_pure_mcts_stats* stats, oaz_pure_node* tree_out, size_t tree_cap);
/* A search's device buffers are one allocation (G x oaz_pure_mcts_tree_capacity nodes + ~100 B per root), and the
 * last one of each device is kept for the next search (a 1 M-search launch's trees are 64 GB); this frees a
 * device's kept buffer (OAZ_ERR_STATE while a search uses it). */
int oaz_pure_mcts_release_workspace(int device);

/* One search per root, each root with its own Mcts{..}: the parameter sweep of bin/mcts_parameter_check.rs (every
 * pairing's games, both sides) as one launch per ply, and the agent's search_time clock. */
typedef struct oaz_pure_mcts_root {      /* 24 bytes: one root's Mcts{..} (ai/mcts/mod.rs:13-30) */
    int32_t  max_playouts;               /* >= 0 */
    int32_t  min_node_visits;            /* >= 0 */
    float    exploration_c;
    uint32_t reserved;                   /* 0 */
    uint64_t stream;                     /* the rollout generator's game word: Philox(seed; stream, playout, 0x9C7A0000, d/4); < 2^32 */
} oaz_pure_mcts_root;

typedef struct oaz_pure_mcts_each_config { /* 32 bytes: what the roots of a call share */
    uint64_t seed;
    int64_t  search_time_ns;             /* 0 = off: exactly max_playouts playouts per root */
    int32_t  rollout_cap;                /* as oaz_pure_mcts_config.rollout_cap */
    int32_t  device;
    int32_t  reserved[2];
} oaz_pure_mcts_each_config;

/* Root g's tree capacity = oaz_pure_mcts_tree_capacity of its (max_playouts, min_node_visits) (0 for a negative
 * one). offsets (optional, G + 1) = their exclusive prefix sums. Returns the total. Host only. */
size_t oaz_pure_mcts_each_capacity(const oaz_pure_mcts_root* par, int G, size_t* offsets);
/* Root g's tree, move and value are those of oaz_pure_mcts_search on that root alone with par[g]'s max_playouts,
 * min_node_visits and exploration_c, the call's seed and rollout_cap, and game_id0 = par[g].stream. A UCT value
 * that is NaN (0 * inf: exploration_c = 0 and an unvisited child) is ordered as the x86 default NaN 0xFFC00000,
 * the smallest key of f32::total_cmp, which is what the reference's arithmetic gives.
 * search_time_ns > 0 is the reference's loop condition (mcts_arena.rs:56-62) read on the device: a root takes the
 * device's constant-rate clock when its search starts, and playout p (0-based) starts only while p < max_playouts
 * and, for p >= min(max_playouts, min_node_visits + 2), while the clock is below the start + search_time_ns.
 * (Defined here: the first min_node_visits + 2 playouts always run, so the root is expanded; the reference
 * panics when its clock cuts earlier.) The clock is read once per playout and nothing waits on it.
 * out_playouts[g] (optional) = the playouts root g ran; its tree is that of a search with max_playouts =
 * out_playouts[g]. tree_out (optional) receives root g's nodes at tree_out + tree_offsets[g], at most
 * tree_offsets[g + 1] - tree_offsets[g] of them; oaz_pure_mcts_each_capacity gives the offsets that hold every
 * tree, and device memory is their total. Every argument is checked before a device is touched (OAZ_ERR_ARG, the
 * message naming the root); G == 0 returns OAZ_OK with zeroed statistics. Device, stream and workspace as
 * oaz_pure_mcts_search. */
int oaz_pure_mcts_search_each(const oaz_state* roots, const oaz_pure_mcts_root* par, int G,
                              const oaz_pure_mcts_each_config* cfg, oaz_move* out_move, float* out_value,
                              int32_t* out_playouts /* optional: playouts each root ran */,
                              oaz_pure_mcts_stats* stats, oaz_pure_node* tree_out /* optional, packed */,
                              const size_t* tree_offsets /* G + 1, required with tree_out */);

/* ---- alpha-beta agent (the fourth opponent of Evaluator::pit, evaluator.rs:276-312) --------------
 * The reference's `AlphaBeta` agent (onitama-game/src/ai/alpha_beta/mod.rs:35-183): fail-soft alpha-beta
 * without move ordering or a table, Red maximising and Blue minimising Evaluation::evaluate
 * (alpha_beta/evaluation.rs:24-110), moves in card slot / from / to order, a cut-off leaving only the
 * current card's moves. generate_move (mod.rs:136-170) deepens iteratively, depth = 1 .. max_depth - 1,
 * and keeps only the last iteration's result, so a run the clock does not cut equals one search to
 * max_depth - 1 plies: that search runs here, one GPU wave per root with one lane per root move.
 * search_time is not enforced by this entry point: oaz_alphabeta_generate_move has the clock (as
 * oaz_pure_mcts_search_each has the pure-MCTS agent's). */
typedef struct oaz_alphabeta_config {
    int32_t max_depth;   /* 6 (alpha_beta/mod.rs:24); the arena's opponent uses 4 (evaluator.rs:303-306).
                            Accepted: 2..6 (the reference panics below 2, mod.rs:161) */
    int32_t device;      /* HIP device the search runs on (its own stream; other work on it is not waited for) */
    int32_t reserved[2];
} oaz_alphabeta_config;

typedef struct oaz_alphabeta_stats {
    uint64_t positions;              /* alpha_beta calls over all roots (mod.rs:46), the last iteration's only */
    uint64_t max_positions_per_root;
    uint64_t roots_without_move;     /* roots answered with the pass move (the reference panics, mod.rs:165-167) */
} oaz_alphabeta_stats;

void oaz_alphabeta_config_default(oaz_alphabeta_config* cfg);   /* AlphaBeta::default, mod.rs:21-28 */
/* Evaluation::evaluate (evaluation.rs:24-90) on the host (no GPU): colour = s[i].to_move, move_result[i] as
 * MoveResult, or move_result = NULL for None. The kernel evaluates leaves with the same function body. */
int oaz_alphabeta_evaluate(const oaz_state* s, const uint8_t* move_result, int n, int32_t* out);
/* One search per root (colour = root.to_move) to max_depth - 1 plies (AlphaBeta::generate_move, mod.rs:136-170,
 * over alpha_beta, mod.rs:36-132); out_score = best_score (i32). A root without a legal move returns the pass
 * move (from = to = 25, piece 0, slot = the mover's first card) and the untouched best_score (INT32_MIN for
 * Red, INT32_MAX for Blue). Runs on cfg->device on a stream of its own with buffers allocated and freed per
 * call (36 B per root); the calling thread's current HIP device is restored before the call returns.
 * max_depth outside 2..6 is OAZ_ERR_ARG, checked before any device is touched. */
int oaz_alphabeta_search(const oaz_state* roots, int G, const oaz_alphabeta_config* cfg,
                         oaz_move* out_move, int32_t* out_score, oaz_alphabeta_stats* stats);

/* Agent::generate_move (mod.rs:136-170) with its clock and up to the tournament's max_depth 8
 * (bin/tournament.rs:107-110), as a split search: the first `split` plies of every root are laid out as levels
 * of nodes in move order, every node of the last level (an "item") is searched by one GPU lane with the full
 * window and the plies that remain, and the exact values are folded back up with the reference's strict
 * comparisons. Moves and scores equal oaz_alphabeta_search's (and the sequential search's) at every split;
 * only the positions visited differ (about 1.7x, 3.8x, 5.9x the sequential search's at split 1, 2, 3). */
typedef struct oaz_alphabeta_agent_config {
    int32_t max_depth;       /* 2..8 (tournament.rs:107-110 uses 8) */
    int32_t device;
    int64_t search_time_ns;  /* 0 = off: the one search to max_depth - 1 plies (as oaz_alphabeta_search) */
    int32_t split;           /* 0 = auto (from G and the plies), 1..3; clamped to plies - 1, at least 1 */
    int32_t reserved[3];
} oaz_alphabeta_agent_config; /* 32 bytes */

typedef struct oaz_alphabeta_agent_stats {
    uint64_t positions, max_positions_per_root, roots_without_move; /* as oaz_alphabeta_stats, last iteration */
    uint64_t items;          /* frontier items searched, last iteration */
    int32_t iterations;      /* iterations run */
    int32_t plies;           /* plies of the last iteration: the result is that search's */
    int32_t split;           /* S used by the last iteration */
    int32_t reserved;
    double elapsed_ms;       /* the whole call on the host's monotonic clock */
} oaz_alphabeta_agent_stats; /* 56 bytes */

void oaz_alphabeta_agent_config_default(oaz_alphabeta_agent_config* cfg);   /* max_depth 6, device 0, 1 s, auto split */
/* One answer per root (colour = root.to_move), out_move / out_score / the pass move as oaz_alphabeta_search's.
 * The clock is the reference's loop (mod.rs:145-156): iteration d = 1, 2, .. (a search to d plies) starts only
 * while d < max_depth and the time since the call began is below search_time_ns; the time is read on the host
 * between iterations, a started iteration is never abandoned, and the result is the last iteration's. The
 * first iteration always runs (defined here: the reference unwraps None when the clock has run out before
 * it). The G roots of a call share the clock and all reach the same depth (stats->plies), so a large batch
 * under a short search_time_ns is searched less deeply than one root would be (as oaz_config.search_time_ns).
 * With search_time_ns == 0 only the last iteration runs, because iterations carry nothing over.
 * Runs on cfg->device on a stream of its own with buffers allocated and freed per call (49 B per node of
 * the split levels; the roots of a large call are searched a few at a time so that a launch holds about 4 M
 * items); the calling thread's current HIP device is restored before the call returns. OAZ_ERR_ARG, checked
 * before any device is touched: a null pointer, max_depth outside 2..8, split outside 0..3, a negative
 * search_time_ns, a root that is not a valid state. An explicit split that puts more than 2^27 nodes on one
 * level is OAZ_ERR_CAPACITY. */
int oaz_alphabeta_generate_move(const oaz_state* roots, int G, const oaz_alphabeta_agent_config* cfg,
                                oaz_move* out_move, int32_t* out_score, oaz_alphabeta_agent_stats* stats);

/* ---- arena: a fight played on the device (Evaluator, alphazero-training/src/evaluator.rs) -----------
 * fight (evaluator.rs:355-399) with all game_amnt games advanced together and their states resident on the
 * GPU: every ply the active games are routed to the side that moves in them (ascending game index), each
 * side answers its games in one batched search, and the moves are applied on the device. Game k is dealt
 * oaz_deal_deck(seed, k) (or the fixed deck) and starts from oaz_initial_state, the neutral card's colour
 * moving first (game_state.rs:37-45), or from cfg->start[k]; the agent plays Red in even
 * games and Blue in odd ones (`agents.reverse()`, evaluator.rs:397). A pass (from == 25; the searches'
 * answer for a root without a legal move) rotates cards[slot] with the neutral card and flips the side to
 * move (state.rs:139-142). A game ends on a win, or after the ply on which the budget (max_plies, one less
 * after every ply) was already negative (evaluator.rs:376-389: 152 plies at max_plies 150, 2 at 0, 1 at -1).
 * Elo and the counters are folded on the host in game order after the last ply (FightStatistics::update,
 * evaluator.rs:52-99), so the statistics equal the reference's one-game-after-the-other loop. */
enum {                       /* the Agent implementations a side can be */
    OAZ_AGENT_ALPHAZERO = 0, /* AlphaZeroMcts, alphazero_mcts/mod.rs:122-161 (evaluator.rs:198-204) */
    OAZ_AGENT_RANDOM = 1,    /* Random, onitama-game/src/ai/random.rs:11-43 */
    OAZ_AGENT_PURE_MCTS = 2, /* Mcts, onitama-game/src/ai/mcts/mod.rs:37-52 (evaluator.rs:340-345) */
    OAZ_AGENT_ALPHABETA = 3  /* AlphaBeta, onitama-game/src/ai/alpha_beta/mod.rs:136-170 (evaluator.rs:303-306) */
};

typedef struct oaz_arena_agent {
    int32_t kind;
    int32_t reserved;
    oaz_engine* engine;             /* ALPHAZERO: a created engine on cfg->device (its weights: oaz_load_weights; or OAZ_EVAL_HASH),
                                       searched with its current sims / c_puct / noise / search_time settings. Both
                                       sides may name the same engine: their searches of a ply then run one after
                                       the other */
    uint64_t seed;                  /* RANDOM: the Philox key of oaz_random_agent_move */
    oaz_pure_mcts_config mcts;      /* PURE_MCTS: seed inside; device and game_id0 are set by the arena: game_id0 =
                                       c << 20 for this side's c-th search of the fight, root g of a search being
                                       the side's g-th game in ascending game index */
    oaz_alphabeta_config alphabeta; /* ALPHABETA (device is set by the arena) */
} oaz_arena_agent; /* 88 bytes */

typedef struct oaz_arena_config { /* EvaluatorConfig, evaluator.rs:120-137 (winrate_percent is the caller's) */
    int32_t game_amnt;            /* 20 */
    int32_t max_plies;            /* 150 */
    int32_t fixed_deck;           /* 1: every game uses deck[]; 0: game k is dealt oaz_deal_deck(seed, k) */
    int32_t device;               /* the HIP device the fight runs on */
    uint8_t deck[5];
    uint8_t pad[3];
    uint64_t seed;
    const oaz_state* start;       /* optional (NULL: deal): game k starts from start[k], its to_move moving first (an
                                     opening book, a test position); deck, fixed_deck and seed are then unused */
} oaz_arena_config; /* 40 bytes */

typedef struct oaz_fight_stats { /* FightStatistics, evaluator.rs:37-110 (the agent is "a") */
    double rating_a, rating_b;
    double winrate;              /* wins / games (update_winrate, evaluator.rs:101-109); 0 before the first game */
    double color_winrate[2];     /* as Red, as Blue; NaN for a colour without games once a game was folded (Rust's 0 / 0) */
    uint32_t wins, loses, draws;
    uint32_t color_wins[2], color_loses[2], color_draws[2];
    uint32_t reserved;
    uint64_t plies_total;        /* moves made over all games (oaz_arena_fight only) */
    uint64_t passes;             /* of them passes (oaz_arena_fight only) */
} oaz_fight_stats; /* 96 bytes */

void oaz_arena_config_default(oaz_arena_config* cfg);   /* EvaluatorConfig::default, evaluator.rs:129-136 */
/* EloRating::elo_change (elo_rating.rs:56-71; K = 32, C = 1 / 400). Host only. */
void oaz_elo_change(double ra, double rb, int a_won, double* ra_out, double* rb_out);
/* FightStatistics::update (evaluator.rs:52-99) folded over n MoveResult codes in game order, game k played by the
 * agent as Red when k is even; anything but a win is a draw. history (optional): n x 4 doubles (before_a,
 * after_a, before_b, after_b), the RatingChange records (evaluator.rs:29-35). Host only. */
int oaz_fight_stats_fold(const uint8_t* results, int n, double rating_a, double rating_b, oaz_fight_stats* out,
                         double* history);
/* Random::generate_move (ai/random.rs:11-43) for global game `game` at ply `ply` of the mover s->to_move: the two
 * draws are words 0 and 1 of Philox4x32-10(seed; game lo, game hi, 0x52414E44, ply): card_idx = (w0 * 2) >> 32
 * among the mover's two cards, then move (w1 * n) >> 32 of that card's n legal moves in generate_legal_moves
 * order (state.rs:301-378; from, to ascending). out->slot = card_idx (0 / 1 for Blue too, random.rs:39); with
 * n == 0 the move is {from 0, to 5, pawn} (random.rs:27-33). Host only; the arena's kernel runs the same body. */
int oaz_random_agent_move(uint64_t seed, uint64_t game, uint32_t ply, const oaz_state* s, oaz_move* out);
/* The largest batch each side answers in a fight of cfg (out[0] the agent's, out[1] the opponent's): the games
 * move in lock step, so a side moves in the games whose first mover (the neutral card's colour,
 * game_state.rs:37-45) it is on even plies and in the others on odd ones: ceil(game_amnt / 2) for a fixed
 * deck, up to game_amnt for random deals. An ALPHAZERO side's engine needs at least that many `games`. Host only. */
int oaz_arena_capacity(const oaz_arena_config* cfg, int32_t out[2]);
/* fight (evaluator.rs:355-399). results / plies (optional, game_amnt each): every game's last MoveResult (a
 * draw is OAZ_CAPTURE or OAZ_IN_PROGRESS) and the moves it made; history as oaz_fight_stats_fold's. Runs on
 * cfg->device on streams of its own and the engines'; the sides' searches of a ply overlap unless they share an
 * engine. PURE_MCTS and ALPHABETA sides go through oaz_pure_mcts_search / oaz_alphabeta_search with their roots
 * and moves staged in pinned host memory (24 B down, 4 B up per root and ply). Calls on disjoint engines may
 * run on several host threads at once. The calling thread's current HIP device is restored before the call
 * returns. Checked before any device is touched: null cfg / agent / opponent / stats or game_amnt < 0, an
 * unknown kind, ALPHAZERO without an engine or with an engine on another device, a
 * fixed deck with a card >= 16 or a repeated card, a start position that is not a valid state,
 * alphabeta.max_depth outside 2..6 (OAZ_ERR_ARG), and an
 * engine with fewer `games` than oaz_arena_capacity asks for (OAZ_ERR_CAPACITY). game_amnt == 0 returns
 * empty statistics without touching a device. */
int oaz_arena_fight(const oaz_arena_config* cfg, const oaz_arena_agent* agent, const oaz_arena_agent* opponent,
                    double agent_rating, double opponent_rating, oaz_fight_stats* stats, uint8_t* results,
                    int32_t* plies, double* history);

/* ---- arena: a fight of any size on a fixed pool of refilled game slots ---------------------------------
 * oaz_arena_fight with S = min(slots, game_amnt) game slots instead of one per game, so that an ALPHAZERO side's
 * engine holds trees for S slots, not for game_amnt games, and late plies do not search ever smaller batches.
 * The schedule, with `next` the first game not dealt yet:
 *   1. slot i < S starts game i; next = S;
 *   2. a round routes the active slots to the side that moves in them (ascending slot index), each side with
 *      at least one root answers its batch in one search, and the moves are applied, as in oaz_arena_fight;
 *   3. before the next round's route every slot that finished stores its result (last MoveResult, plies,
 *      passes) under its game index;
 *   4. the finished slots then take games next, next + 1, ... in ascending slot index while next < game_amnt:
 *      the game's start position (oaz_deal_deck(seed, k) + oaz_initial_state, the fixed deck, or start[k]),
 *      budget max_plies, no plies or passes made;
 *   5. a finished slot that gets no game stays empty and is not harvested again;
 *   6. the fight ends when a route finds no root for either side.
 * Every active slot moves exactly once per round, so `rounds` is a function of the games' lengths and S alone.
 * Results, plies and history are indexed by game and Elo is folded in game order, as in oaz_arena_fight. Extra
 * device memory: 33 B per game (start state 24, result 1 + 4 + 4).
 * Equalities: with slots >= game_amnt nothing is refilled and the call is oaz_arena_fight ply for ply, the
 * pure-MCTS streams included. With fewer slots, a side whose answer depends only on the position (ALPHAZERO
 * with root noise off, ALPHABETA without a clock) or on (game, ply) (RANDOM) plays every game as in
 * oaz_arena_fight, so results, plies and statistics are equal game for game. Not equal: an ALPHAZERO side with
 * root noise on (the noise is keyed by the engine's search count, so by the schedule) or stopped by its
 * search_time (one clock per batch), and a PURE_MCTS side, which keeps the stream rule with "slot" for "game":
 * game_id0 = c << 20 for the side's c-th search of the fight, root g being the side's g-th root in ascending slot
 * index. That fight is still deterministic. The rollout generator's game word is 32 bits, so a PURE_MCTS side's
 * streams recur after 4 096 searches of one fight. */
typedef struct oaz_arena_slots_stats {
    uint64_t rounds;        /* loop iterations in which at least one game moved */
    uint64_t searches[2];   /* rounds in which the agent / the opponent had at least one root */
    uint32_t max_batch[2];  /* the largest batch each side answered */
    uint32_t slots;         /* slots used: min(slots, game_amnt) */
    uint32_t reserved;
} oaz_arena_slots_stats; /* 40 bytes */

/* oaz_arena_capacity for a fight on `slots` slots: its values for slots >= game_amnt, else out[0] = out[1] =
 * slots (slots at different plies can all be one side's turn). An ALPHAZERO side's engine needs at least that
 * many `games`. slots < 1 is OAZ_ERR_ARG. Host only. */
int oaz_arena_slots_capacity(const oaz_arena_config* cfg, int32_t slots, int32_t out[2]);
/* oaz_arena_fight on a pool of slots (above): the same arguments with the same meaning and the same checks
 * before any device is touched, with oaz_arena_slots_capacity for oaz_arena_capacity; in addition slots < 1 is
 * OAZ_ERR_ARG. slot_stats is optional. game_amnt == 0 returns empty statistics and rounds == 0 without touching
 * a device. */
int oaz_arena_fight_slots(const oaz_arena_config* cfg, int32_t slots, const oaz_arena_agent* agent,
                          const oaz_arena_agent* opponent, double agent_rating, double opponent_rating,
                          oaz_fight_stats* stats, uint8_t* results, int32_t* plies, double* history,
                          oaz_arena_slots_stats* slot_stats);

/* ---- left-right reflection ---------------------------------------------------------
 * Onitama is invariant under the reflection in the c-file when every card is replaced by its reflected card: the
 * start position (state.rs:24-45), the temples (state.rs:48-49: c5 and c1) and the rules are symmetric, and the
 * attack maps obey reflect(ATTACK_MAPS[c][k][f]) == ATTACK_MAPS[c][C[k]][R(f)] (card.rs:476-604). Neither the
 * reference nor its training loop uses this; it is what doubles a self-play buffer for free.
 *   square   R(i) = 5 * (i / 5) + 4 - i % 5 for i < 25; R(25) = 25 (the pass move's from = to = 25)
 *   bitboard the bit of square i (1u << (31 - i), common/mod.rs:2-16) moves to the bit of R(i); bits 6..0 stay
 *   card     C = 0 1 3 2 4 5 7 6 8 9 10 12 11 13 15 14 (ORIGINAL_CARDS order, card.rs:465-468): Frog<->Rabbit,
 *            Goose<->Rooster, Horse<->Ox, Eel<->Cobra, the other eight fixed; derived at compile time from the
 *            attack table as the unique card obeying the law
 *   state    kings[c], pawns[c] reflected, cards[k] = C[cards[k]] in the same deck slot (deck.rs:14-18); to_move
 *            and pad unchanged
 *   move     from and to through R; piece and slot unchanged (a reflected card keeps its slot)
 *   sample   the state as above; pi'[k * 25 + R(t)] = pi[k * 25 + t] for k = 0, 1 (pi is keyed by hand slot and
 *            `to`, calculate_priors, mcts_arena.rs:104-124); z unchanged. Bytes are moved, never recomputed:
 *            applying the transformation twice returns the input byte for byte.
 * Host helpers (no GPU). out == in is allowed; n == 0 is OAZ_OK. A card id >= 16 or a square > 25 in any element
 * is OAZ_ERR_ARG (as a null pointer or n < 0), and nothing is written then. */
int oaz_reflect_card(int card);   /* C[card]; -1 outside 0..15 */
int oaz_reflect_states_host(const oaz_state* in, int n, oaz_state* out);
int oaz_reflect_moves_host(const oaz_move* in, int n, oaz_move* out);
int oaz_reflect_samples_host(const oaz_sample* in, size_t n, oaz_sample* out);
/* The same as oaz_reflect_samples_host on the GPU (host pointers, the thread's current device, as oaz_encode):
 * the records go through device scratch buffers and one kernel whose lanes stride over the 57 words of
 * consecutive records. The same argument checks, made on the host before a device is touched. */
int oaz_reflect_samples(const oaz_sample* in, size_t n, oaz_sample* out);
/* oaz_trainer_set_batches with a flag per index entry (n_batches x batch bytes, 0 or 1; NULL = all 0, which is
 * oaz_trainer_set_batches): a flagged entry makes the step's gather produce the input planes, pi row and z of
 * the reflected sample (create_tensor_from_state, common.rs:26-80, of the reflected state), inside the one
 * gather launch and without a reflected copy of the buffer, on owned and on bound samples (which are only read)
 * and on every step path (backward, apply, train). A flag other than 0 or 1 is OAZ_ERR_ARG, as a bad index is,
 * and leaves the uploaded batches as they were. Sample indices must then be below 2^31, which int32 makes them. */
int oaz_trainer_set_batches_reflect(oaz_trainer* t, const int32_t* idx, const uint8_t* reflect, int n_batches,
                                    int batch);

/* ---- replay buffer: a window of iterations on the device, duplicates merged --------
 * The training data of the last `window` appends (one append = one segment = one iteration's self-play), kept
 * on the device in arrival order and capped by `capacity` records; and a merged view of it in which records
 * of equal position are one record with the mean pi and the mean z. The reference keeps one iteration's Vec
 * (train.rs:241-250; TrainConfig.buffer_size is only its capacity, train.rs:128) and trains on every copy.
 *
 * The merge rule. A record's key is the 22 bytes kings[2], pawns[2], cards[5], to_move of oaz_sample.state (pad
 * is not part of it). Records of equal key form a group; its representative is the member of smallest arrival
 * index and its multiplicity m its size. The output holds one record per group, ordered by the representative's
 * arrival index, and mult[] (uint32). m == 1: the input record byte for byte. m > 1: state = the
 * representative's 24 bytes (its pad included); for each of the 50 pi entries and for z, with
 * F(x) = rint((double)x * 2^32) as a 64-bit integer (unsigned for pi, signed for z; round half to even) and
 * S = the integer sum of F(x) over the group, the entry is (float)((double)S / ((double)m * 4294967296.0)): one
 * correctly rounded double division, then round to nearest even to float. Integer sums do not depend on the
 * order, so the device's bytes are the host's. pi is assumed to lie in [0, 1] and z in [-1, 1] (what self-play
 * writes); values outside, NaN included, are not checked and give unspecified entries in merged records only.
 *
 * The window. Each append is one segment, n == 0 included (an iteration without records still ages the window).
 * A segment of more than `capacity` records is OAZ_ERR_CAPACITY and changes nothing. After an append the oldest
 * segments are dropped while there are more than `window` of them, then while the records exceed `capacity`
 * and more than one segment is left. `tag` (the loop passes the iteration number) is kept with the segment and
 * appears in error texts only.
 *
 * Threading as the engine's: one thread at a time per buffer; every entry runs on the buffer's device and
 * restores the calling thread's current device. */
typedef struct oaz_replay oaz_replay;
typedef struct oaz_replay_config {
    uint64_t capacity;     /* records; default 180000 = TrainConfig.buffer_size (train.rs:128); < 2^31 */
    int32_t  window;       /* segments (iterations) kept; default 1 */
    int32_t  device;
    uint32_t table_slots;  /* 0 = auto: smallest power of two >= 2 n; else a power of two > n of the view being built, OAZ_ERR_ARG otherwise */
    uint32_t pad;
} oaz_replay_config; /* 24 bytes */
typedef struct oaz_replay_stats {
    uint64_t segments, records;                 /* in the window now */
    uint64_t unique, max_mult;                  /* of the last merged view */
    uint64_t appended, evicted;                 /* records, since creation */
    uint64_t probes;                            /* key comparisons of the last merge */
} oaz_replay_stats; /* 56 bytes */

void oaz_replay_config_default(oaz_replay_config* cfg);
/* NULL (oaz_last_error): capacity 0 or >= 2^31, window < 1, no such device. */
oaz_replay* oaz_replay_create(const oaz_replay_config* cfg);
void oaz_replay_destroy(oaz_replay* r);
/* One segment from host memory, from device memory of the buffer's device (read on the buffer's stream; the
 * caller's writes to it are complete), or all of an engine's buffered samples device to device (the engine's
 * buffer is empty afterwards; *n_out, optional, = records taken; an engine on another device is OAZ_ERR_ARG). */
int oaz_replay_append_host(oaz_replay* r, const oaz_sample* host, size_t n, int64_t tag);
int oaz_replay_append_device(oaz_replay* r, const oaz_sample* dev, size_t n, int64_t tag);
int oaz_replay_append_engine(oaz_replay* r, oaz_engine* eng, int64_t tag, size_t* n_out);
/* The window as device memory. merge == 0: its records, contiguous, in arrival order; *dev_mult = NULL.
 * merge == 1: the merged records and their multiplicities (the rule above). Returns after the buffer's stream
 * is synchronised, so work on any other stream may read; the pointers hold until the next append, view, fetch
 * or destroy. An empty window gives *n = 0 and launches nothing. dev_mult may be NULL. */
int oaz_replay_view(oaz_replay* r, int merge, const oaz_sample** dev, size_t* n, const uint32_t** dev_mult);
/* oaz_replay_view copied to host memory: out[cap], mult[cap] (optional; all 1 with merge == 0).
 * OAZ_ERR_CAPACITY when the view holds more than cap records; *n_out is the view's size either way. */
int oaz_replay_fetch(oaz_replay* r, int merge, oaz_sample* out, uint32_t* mult, size_t cap, size_t* n_out);
int oaz_replay_stats_get(oaz_replay* r, oaz_replay_stats* out);
/* The last merged view's device time by phase, in milliseconds (HIP events on the buffer's stream): key pass,
 * insert, lookup, scan + compact, group (count, scan, member lists), emit. All 0 before the first merge. */
enum { OAZ_REPLAY_PHASES = 6 };
int oaz_replay_merge_times(oaz_replay* r, double ms[OAZ_REPLAY_PHASES]);
/* The merge rule in plain C++ on the host (no GPU): out[n], mult[n] (optional), *n_out = groups. out may not
 * overlap in. */
int oaz_replay_merge_host(const oaz_sample* in, size_t n, oaz_sample* out, uint32_t* mult, size_t* n_out);

/* ---- held-out evaluation: a split by position and an eval-mode pass -----------------
 * What lets two training recipes be compared on records neither trained on. Added entries: OAZ_ABI_VERSION
 * stays 5.
 *
 * The split rule. A record is held out as a function of its position only: the key is the replay buffer's (the
 * 22 bytes kings[2], pawns[2], cards[5], to_move as six little-endian 32-bit words k0 .. k5, the pad bytes 0),
 * so all copies of a position, in every iteration of a replay window, and a merged record, fall on one side.
 * With the library's Philox4x32-10 (key; four counter words -> four words w0 .. w3):
 *   a = philox(seed; k0, k1, k2, k3)
 *   b = philox(a.w0 | a.w1 << 32; k4, k5, 0x484F4C44 "HOLD", 0)
 *   held out iff (b.w0 & 0xFFFF) < per_65536, per_65536 in 0 .. 65536 (0: no record, 65536: every record).
 * pi and z are not looked at. per_65536 > 65536, or a null pointer with n > 0, is OAZ_ERR_ARG; n == 0 is OAZ_OK.
 * oaz_holdout_pick and oaz_holdout_mask_host need no GPU. oaz_holdout_mask runs a kernel over n records that are
 * in the memory of `device` (a replay view, oaz_samples_export_device; the caller's writes to them are complete)
 * and copies the n mask bytes to host_out; the records are only read and do not move. */
int oaz_holdout_pick(uint64_t seed, const oaz_state* s, uint32_t per_65536); /* 0 / 1; < 0 on bad arguments */
int oaz_holdout_mask_host(const oaz_sample* in, size_t n, uint64_t seed, uint32_t per_65536, uint8_t* out);
int oaz_holdout_mask(const oaz_sample* dev, size_t n, uint64_t seed, uint32_t per_65536, int device,
                     uint8_t* host_out);

/* The eval-mode pass: the trainer's fp32 forward with every BN layer on its running statistics and bn_eps (the
 * network as the engine plays it), over entries of the trainer's loaded or bound samples. Sums, not means: the
 * caller divides. */
typedef struct oaz_eval_stats {
    uint64_t n;             /* entries evaluated */
    uint64_t decided;       /* entries with z != 0 */
    uint64_t top1;          /* entries where pi[argmax p] == max pi (argmax p: the lowest index on ties) */
    uint64_t sign;          /* decided entries with v * z > 0 */
    double value_sq;        /* sum (z - v)^2, elementwise (not the training loss's [B,B] broadcast form, which
                               depends on the batch's composition) */
    double policy_ce;       /* sum over entries of -sum_k pi_k log p_k; terms with pi_k == 0 contribute 0 */
    double target_entropy;  /* sum of -sum_k pi_k log pi_k; policy_ce - target_entropy = sum KL(pi || p) */
    double reserved;        /* 0 */
} oaz_eval_stats; /* 64 bytes */
/* idx: n host indices into the samples, NULL = records 0 .. n-1. reflect: n flags with the meaning of
 * oaz_trainer_set_batches_reflect, NULL = none; predict returns a flagged entry's policy in the reflected
 * coordinates. Any n >= 0: the call runs chunks of at most max_batch entries, the last one padded to a multiple
 * of 16 with the padding masked out of every sum and output. An index out of range (or, with idx == NULL,
 * n above the sample count) or a flag other than 0 / 1 is OAZ_ERR_ARG; no samples loaded or bound is
 * OAZ_ERR_STATE.
 * The pass changes nothing a training step reads or reports: parameters, running statistics, momentum buffers,
 * the gradient buffer, the loss accumulators and the uploaded index matrix stay bit for bit. It runs on the
 * trainer's stream, after the weight-gradient stream's work, and returns with the stream synchronised.
 * An entry's outputs depend on that entry alone: predict's p and v of a record are the same bits wherever it
 * stands in idx, whatever its neighbours and whatever max_batch; evaluate writes a term per entry and adds them
 * in one fixed order, so its sums are the same bytes for every max_batch.
 * policy: n x 50 floats (pi's layout), value: n floats. */
int oaz_trainer_evaluate(oaz_trainer* t, const int32_t* idx, size_t n, const uint8_t* reflect, oaz_eval_stats* out);
int oaz_trainer_predict(oaz_trainer* t, const int32_t* idx, size_t n, const uint8_t* reflect, float* policy,
                        float* value);

#ifdef __cplusplus
}
#endif
#endif /* ONITAMA_AZ_H */
