// oaz_engine.cpp — host side of the C ABI (include/onitama_az.h).
//
// Owns the device buffers of one engine (one GPU), orchestrates the per-simulation kernel
// sequence  select -> evaluate -> expand/backup  for all G games in lock step, and the
// per-move finalisation (search result or self-play ply). No compute happens on the host
// except weight folding/packing (oaz_pack.cpp), deck dealing for host helpers and sqrt tables.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <time.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/onitama_az.h"
#include "oaz_device.h"
#include "oaz_host.h"
#include "oaz_kernels.h"
#include "oaz_pack.h"
#include "oaz_weights_layout.h"

using namespace oaz;

static_assert(offsetof(oaz_config, search_time_ns) == 104 && offsetof(oaz_config, reuse_visits) == 116 &&
                  sizeof(oaz_config) == 120,
              "oaz_config layout (ABI 4; reuse_visits took the reserved word)");
static_assert(offsetof(oaz_config, leaf_batch) == 70 && offsetof(oaz_config, seed) == 72,
              "oaz_config layout (leaf_batch took a pad byte)");

// ---- errors ---------------------------------------------------------------------------------
static thread_local std::string g_err;

int oaz_set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" int oaz_abi_version(void) { return OAZ_ABI_VERSION; }
extern "C" const char* oaz_last_error(void) { return g_err.c_str(); }

extern "C" void oaz_config_default(oaz_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->blocks = 5;          // bin/train.rs:57-61
    c->channels = 64;
    c->in_planes = 21;
    c->sims = 400;          // bin/train.rs:53
    c->c_puct = 5.0;        // bin/train.rs:54
    c->train_noise = 1;     // bin/train.rs:55
    c->max_plies = 150;     // train.rs:152
    c->dirichlet_alpha = 0.03;
    c->dirichlet_eps = 0.25;
    c->games = 4096;
    c->evaluator = OAZ_EVAL_NN;
    // the fp32 network by the fp16x3 split (within 1e-5 of fp32, tests/test_gpu.py): the precision the
    // one-launch Agent search (k_search_lat) and the C3 headline run; OAZ_FP32 is the exact-fp32 MFMA kernel
    c->precision = OAZ_FP32_SPLIT16;
    c->fixed_deck = 0;
    for (int i = 0; i < 5; ++i) c->deck[i] = (uint8_t)i;  // ORIGINAL_CARDS[0..5]
    c->seed = 20260101ull;
    c->rank = 0;
    c->world = 1;
}

extern "C" int oaz_device_count(int* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (n) *n = (e == hipSuccess) ? c : 0;
    if (e != hipSuccess) return oaz_set_err(OAZ_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return 0;
}

static double now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e9 + (double)ts.tv_nsec;
}

// ---- host helpers -----------------------------------------------------------------------------
extern "C" void oaz_attack_maps(uint32_t out[2 * 16 * 25]) {
    memcpy(out, kAttackHost.m, sizeof(kAttackHost.m));
}

extern "C" size_t oaz_nn_device_bytes(int blocks, int precision) {
    if (blocks < 0 || blocks > 64 || precision < OAZ_FP32 || precision > OAZ_FP32_SPLIT16) return 0;
    return nn_packed_floats(blocks, precision) * sizeof(float);
}

extern "C" size_t oaz_weight_count(int blocks, int channels, int in_planes) {
    return wl::layout(blocks, (size_t)channels, (size_t)in_planes).total;
}

// Weights and biases U(+-1/sqrt(fan_in)), one draw per element in blob order; BN gamma 1, beta 0, mean 0, var 1.
extern "C" int oaz_random_weights(uint64_t seed, int blocks, float* out, size_t n) {
    const wl::Layout L = wl::layout(blocks);
    if (!out || n != L.total || blocks < 0) return oaz_set_err(OAZ_ERR_ARG, "random_weights: need %zu floats", L.total);
    uint64_t ctr = 0;
    for (const wl::Tensor& t : L.tensors) {
        const float bound = t.fan_in ? (float)(1.0 / sqrt((double)t.fan_in)) : 0.0f;
        for (size_t i = 0; i < t.numel; ++i) {
            if (!t.fan_in) {
                out[t.offset + i] = t.fill;
                continue;
            }
            const uint64_t r = splitmix64(seed ^ splitmix64(ctr++));
            const double u = (double)(r >> 11) * (1.0 / 9007199254740992.0);
            out[t.offset + i] = (float)((2.0 * u - 1.0) * bound);
        }
    }
    return 0;
}

extern "C" void oaz_deal_deck(uint64_t seed, uint64_t game_id, uint8_t out[5]) {
    deal_deck(seed, game_id, out);
}

extern "C" int oaz_slot_game_ids(int rank, int world, int games, uint64_t seq, uint64_t* out) {
    if (!out || games < 1 || world < 1 || rank < 0 || rank >= world)
        return oaz_set_err(OAZ_ERR_ARG, "slot_game_ids: rank %d of %d, %d games", rank, world, games);
    for (int g = 0; g < games; ++g) out[g] = slot_game_id(seq, (uint32_t)world, (uint32_t)rank, (uint32_t)games, (uint32_t)g);
    return 0;
}

extern "C" void oaz_initial_state(const uint8_t deck[5], oaz_state* out) {
    if (!deck || !out) return;
    initial_state(deck, *out);
}

extern "C" double oaz_root_noise(uint64_t seed, uint64_t game_id, uint32_t ply, uint32_t sim, uint32_t draw,
                                double alpha, int nchild) {
    return (double)root_noise(seed, game_id, (ply << 16) | (sim & 0xFFFFu), draw, alpha, nchild);
}

extern "C" int oaz_temperature_pick(uint64_t seed, uint64_t game_id, uint32_t ply, const uint32_t* visits, int K) {
    if (!visits) return -1;
    return temperature_draw_child(seed, game_id, ply, visits, K);
}

extern "C" void oaz_hash_eval(const oaz_state* s, float policy[50], float* value) {
    const uint64_t h = hash_state(*s);
    for (int i = 0; i < 50; ++i) policy[i] = hash_policy(h, i);
    *value = hash_value(h);
}

// ---- left-right reflection on the host (oaz_device.h "left-right reflection") --------------------
extern "C" int oaz_reflect_card(int card) { return card < 0 || card > 15 ? -1 : reflect_card(card); }

static bool reflect_states_ok(const oaz_state* s, size_t n, size_t stride) {
    for (size_t i = 0; i < n; ++i)
        if (!reflect_state_ok(*reinterpret_cast<const oaz_state*>(reinterpret_cast<const char*>(s) + i * stride)))
            return false;
    return true;
}

extern "C" int oaz_reflect_states_host(const oaz_state* in, int n, oaz_state* out) {
    if (!in || !out || n < 0) return oaz_set_err(OAZ_ERR_ARG, "reflect_states: bad arguments");
    if (!reflect_states_ok(in, (size_t)n, sizeof(oaz_state)))
        return oaz_set_err(OAZ_ERR_ARG, "reflect_states: a card id is not below 16");
    for (int i = 0; i < n; ++i) reflect_state(in[i], out[i]);
    return 0;
}

extern "C" int oaz_reflect_moves_host(const oaz_move* in, int n, oaz_move* out) {
    if (!in || !out || n < 0) return oaz_set_err(OAZ_ERR_ARG, "reflect_moves: bad arguments");
    for (int i = 0; i < n; ++i)
        if (in[i].from > 25 || in[i].to > 25) return oaz_set_err(OAZ_ERR_ARG, "reflect_moves: move %d: square above 25", i);
    for (int i = 0; i < n; ++i) {
        oaz_move m = in[i];
        m.from = (uint8_t)reflect_sq(m.from);
        m.to = (uint8_t)reflect_sq(m.to);
        out[i] = m;
    }
    return 0;
}

static int reflect_samples_check(const oaz_sample* in, size_t n, const oaz_sample* out) {
    if (!in || !out) return oaz_set_err(OAZ_ERR_ARG, "reflect_samples: null pointer");
    if (!reflect_states_ok(&in->state, n, sizeof(oaz_sample)))
        return oaz_set_err(OAZ_ERR_ARG, "reflect_samples: a card id is not below 16");
    return 0;
}

extern "C" int oaz_reflect_samples_host(const oaz_sample* in, size_t n, oaz_sample* out) {
    if (int rc = reflect_samples_check(in, n, out)) return rc;
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[kSampleWords], r[kSampleWords];  // a copy first: out may be in
        memcpy(w, &in[i], sizeof(w));
        for (int d = 0; d < kSampleWords; ++d) r[d] = reflect_sample_word(d, w[reflect_sample_src(d)]);
        memcpy(&out[i], r, sizeof(r));
    }
    return 0;
}

// ---- rules context (no engine needed) ----------------------------------------------------------
// One context per device (stream + scratch buffers allocated on that device): the rules entry points run
// on the calling thread's current device, so calls from threads on different GPUs never share buffers.
struct RulesCtx {
    std::mutex mu;
    bool init = false;
    Stream stream;
    DevBuf<oaz_state> a;  // grow-only scratch: states,
    DevBuf<uint32_t> b;   // move masks or input planes (4-byte words),
    DevBuf<oaz_move> c;   // moves,
    DevBuf<uint8_t> d;    // move counts or results
    DevBuf<oaz_sample> e, f;  // records in and out (oaz_reflect_samples)
};
constexpr int kRulesMaxDevices = 64;
// never deleted: no hipFree or hipStreamDestroy while the HIP runtime unloads at process exit (oaz_host.h)
static RulesCtx* const g_rules_dev = new RulesCtx[kRulesMaxDevices];

// The current device's context, locked for the caller (lk), its stream created on first use.
static int rules_begin(RulesCtx** out, std::unique_lock<std::mutex>& lk) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return oaz_set_err(OAZ_ERR_NO_DEVICE, "no HIP device visible (the rules run on the GPU)");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kRulesMaxDevices) return oaz_set_err(OAZ_ERR_ARG, "rules: device %d unsupported", dev);
    RulesCtx& r = g_rules_dev[dev];
    lk = std::unique_lock<std::mutex>(r.mu);
    if (!r.init) {
        if (int rc = r.stream.create()) return rc;
        r.init = true;
    }
    *out = &r;
    return 0;
}

extern "C" int oaz_movegen(const oaz_state* s, int n, uint32_t* masks, oaz_move* moves, uint8_t* counts) {
    if (!s || n < 0) return oaz_set_err(OAZ_ERR_ARG, "movegen: bad arguments");
    if (n == 0) return 0;
    RulesCtx* R = nullptr;
    std::unique_lock<std::mutex> lk;
    if (int rc = rules_begin(&R, lk)) return rc;
    hipStream_t st = R->stream;
    if (int rc = R->a.reserve((size_t)n)) return rc;
    if (int rc = R->b.reserve((size_t)n * 50)) return rc;
    if (int rc = R->c.reserve((size_t)n * OAZ_MAX_MOVES)) return rc;
    if (int rc = R->d.reserve((size_t)n)) return rc;
    HIP_TRY(hipMemcpyAsync(R->a, s, (size_t)n * sizeof(oaz_state), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_movegen(R->a, n, masks ? R->b.get() : nullptr, moves ? R->c.get() : nullptr,
                           counts ? R->d.get() : nullptr, st));
    if (masks) HIP_TRY(hipMemcpyAsync(masks, R->b, (size_t)n * 50 * 4, hipMemcpyDeviceToHost, st));
    if (moves) HIP_TRY(hipMemcpyAsync(moves, R->c, (size_t)n * OAZ_MAX_MOVES * sizeof(oaz_move), hipMemcpyDeviceToHost, st));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, R->d, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int oaz_step(oaz_state* s, const oaz_move* mv, int n, uint8_t* results) {
    if (!s || !mv || n < 0) return oaz_set_err(OAZ_ERR_ARG, "step: bad arguments");
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i)
        if (mv[i].from > 24 || mv[i].to > 24 || mv[i].slot > 3 || mv[i].piece > 1)
            return oaz_set_err(OAZ_ERR_ARG, "step: move %d out of range", i);  // deck.rs:88 assert
    RulesCtx* R = nullptr;
    std::unique_lock<std::mutex> lk;
    if (int rc = rules_begin(&R, lk)) return rc;
    hipStream_t st = R->stream;
    if (int rc = R->a.reserve((size_t)n)) return rc;
    if (int rc = R->c.reserve((size_t)n)) return rc;
    if (int rc = R->d.reserve((size_t)n)) return rc;
    HIP_TRY(hipMemcpyAsync(R->a, s, (size_t)n * sizeof(oaz_state), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(R->c, mv, (size_t)n * sizeof(oaz_move), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_step(R->a, R->c, n, R->d, st));
    HIP_TRY(hipMemcpyAsync(s, R->a, (size_t)n * sizeof(oaz_state), hipMemcpyDeviceToHost, st));
    if (results) HIP_TRY(hipMemcpyAsync(results, R->d, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int oaz_current_state(const oaz_state* s, int n, uint8_t* results) {
    if (!s || !results || n < 0) return oaz_set_err(OAZ_ERR_ARG, "current_state: bad arguments");
    if (n == 0) return 0;
    RulesCtx* R = nullptr;
    std::unique_lock<std::mutex> lk;
    if (int rc = rules_begin(&R, lk)) return rc;
    hipStream_t st = R->stream;
    if (int rc = R->a.reserve((size_t)n)) return rc;
    if (int rc = R->d.reserve((size_t)n)) return rc;
    HIP_TRY(hipMemcpyAsync(R->a, s, (size_t)n * sizeof(oaz_state), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_current_state(R->a, n, R->d, st));
    HIP_TRY(hipMemcpyAsync(results, R->d, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int oaz_encode(const oaz_state* s, int n, float* planes) {
    if (!s || !planes || n < 0) return oaz_set_err(OAZ_ERR_ARG, "encode: bad arguments");
    if (n == 0) return 0;
    RulesCtx* R = nullptr;
    std::unique_lock<std::mutex> lk;
    if (int rc = rules_begin(&R, lk)) return rc;
    hipStream_t st = R->stream;
    if (int rc = R->a.reserve((size_t)n)) return rc;
    if (int rc = R->b.reserve((size_t)n * 525)) return rc;
    HIP_TRY(hipMemcpyAsync(R->a, s, (size_t)n * sizeof(oaz_state), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_encode(R->a, n, (float*)R->b.get(), st));
    HIP_TRY(hipMemcpyAsync(planes, R->b, (size_t)n * 525 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int oaz_reflect_samples(const oaz_sample* in, size_t n, oaz_sample* out) {
    if (int rc = reflect_samples_check(in, n, out)) return rc;
    if (n == 0) return 0;
    if (!launch_reflect_samples) return oaz_set_err(OAZ_ERR_STATE, "reflect_samples: built without its kernel");
    RulesCtx* R = nullptr;
    std::unique_lock<std::mutex> lk;
    if (int rc = rules_begin(&R, lk)) return rc;
    hipStream_t st = R->stream;
    if (int rc = R->e.reserve(n)) return rc;
    if (int rc = R->f.reserve(n)) return rc;
    HIP_TRY(hipMemcpyAsync(R->e, in, n * sizeof(oaz_sample), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_reflect_samples(R->e, n, R->f, st));
    HIP_TRY(hipMemcpyAsync(out, R->f, n * sizeof(oaz_sample), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---- engine ------------------------------------------------------------------------------------
constexpr int kMaxParts = 4;  // run_sims: game parts, each on its own stream (oaz_config.parts)

// What a timed launch counts as in oaz_kernel_times (accumulate's table is in this order).
// K_NOISE: the root noise (second stream); K_COMPACT: leaf compaction; K_BACKUP_SELECT: expand/backup + next
// select (fused), and the one-launch searches.
enum LaunchKind { K_SELECT, K_NN, K_EXPAND, K_FINALIZE, K_NOISE, K_COMPACT, K_BACKUP_SELECT, K_COUNT };

struct TimedLaunch {
    LaunchKind kind;
    Event a, b;
    uint32_t samples;
};

// The facts about the last run_sims (oaz_last_sims, oaz_search_playouts).
struct LastSearch {
    uint32_t G = 0;                  // its games
    uint32_t sims = 0;               // simulations per game (Q7 budget: may be < cfg.sims)
    bool on_device = false;          // Q7 on the device: each game's count is still in sims_run; fetch_sims_run
                                     // reads them once into per_game, and sims is then their maximum
    std::vector<uint32_t> per_game;  // (empty: every game ran `sims`)
};

// The device resources are owning members (oaz_host.h), destroyed in reverse declaration order after
// oaz_destroy synchronised the streams: events (declared last) first, then the buffers, the streams
// (declared first) last. Keep that order when adding a member.
struct oaz_engine {
    oaz_config cfg;
    int device = 0;
    Stream stream;
    Stream stream2;                      // root-noise producer, overlaps the NN kernel
    Stream stream3[kMaxParts - 1];       // the streams of game parts 1.. (oaz_config.parts)
    int cus = 256;                      // compute units of the device (leaf-compaction threshold)
    DevBuf<noise_t> noise;               // [2][noise_chunk][G][kNoiseStride] (f64 draws)
    uint32_t noise_chunk = 16;           // simulations per noise ring slot (noise_chunk_for)
    uint32_t G = 0, cap = 0, pathcap = 0, hcap = 0, out_cap = 0;
    int32_t sims_cap = 0;                // cfg.sims at creation: trees and paths are sized for it
    // trees
    DevBuf<oaz_node> nodes;
    DevBuf<uint32_t> n_nodes, path, depth, leaf;
    DevBuf<oaz_state> leaf_state;
    DevBuf<uint64_t> stats, stats_sum;
    DevBuf<double> sqrt_tab;
    DevBuf<float> policy, value;         // evaluations by compacted row (TreeView::slot)
    DevBuf<uint8_t> need;                // leaf compaction (oaz_kernels.h TreeView)
    DevBuf<uint32_t> slot, bcnt;
    DevBuf<oaz_state> cstate;
    DevBuf<float> weights;
    bool have_weights = false;
    DevBuf<unsigned long long> nn_fallback;  // OAZ_FP32_SPLIT16: tiles recomputed by k_nn_x6 (fp16 range)
    // search mode
    DevBuf<oaz_state> s_roots;
    DevBuf<oaz_move> s_move;
    DevBuf<float> s_pi, s_rootv, s_rootp;
    uint32_t search_calls = 0;
    LastSearch last;
    // Q7 on the device (the one-launch searches): the deadline on the device clock, each game's simulation count
    DevBuf<uint64_t> deadline;
    DevBuf<uint32_t> sims_run;
    int wall_khz = 0;  // hipDeviceAttributeWallClockRate (kHz)
    double t_search0 = 0.0;  // host clock at the start of the current search / ply (0: no budget)
    DevBuf<uint32_t> s_ply;
    // self-play
    DevBuf<oaz_state> root;
    DevBuf<uint32_t> ply, seq;
    DevBuf<uint64_t> game_id;
    DevBuf<uint8_t> active;
    DevBuf<oaz_sample> hist, out;
    DevBuf<unsigned long long> out_count;
    DevBuf<uint32_t> fin;      // SlotView::fin / fin_pos (records of the games that ended in a ply)
    DevBuf<uint64_t> fin_pos;
    // tree reuse (cfg.reuse_visits > 0; nothing is allocated without it): oaz_search_advance's per-game scratch
    // (the caller's moves, the validation codes, the kept visits) and the oaz_reuse_stats counters
    DevBuf<oaz_move> adv_moves;
    DevBuf<int32_t> adv_codes, adv_kept;
    DevBuf<uint64_t> reuse_cnt;
    // leaf-parallel search (cfg.leaf_batch > 0; nothing is allocated without it): the rounds' records per root
    // (ParBufs, oaz_kernels.h)
    DevBuf<uint32_t> par_path, par_depth, par_leaf;
    DevBuf<oaz_state> par_state;
    DevBuf<float> par_policy, par_value;
    DevBuf<uint64_t> par_stats;
    uint32_t par_G = 0;           // roots of the last leaf-parallel search (0: none yet)
    DevBuf<uint64_t> temp_cnt;    // self-play temperature (cfg.temperature_plies > 0 only): oaz_selfplay_temperature_stats
    // playout cap randomization (oaz_selfplay_set_playout_cap; nothing is allocated before a cap is set, and the
    // buffers stay once made): the cap, the per-slot full flag and the two phase masks ([3][G]), the per-slot
    // record count and the two oaz_selfplay_playout_cap_stats counters (CapView, oaz_kernels.h)
    int32_t pc_fast = 0;          // fast_sims (0: no cap)
    uint32_t pc_share = 0;        // the full share in 1/65 536
    DevBuf<uint8_t> pc_flags;
    DevBuf<uint32_t> pc_nrec;
    DevBuf<unsigned long long> pc_cnt;
    uint32_t searched = 0;        // games whose trees are the last oaz_search / oaz_search_resume's (0: self-play ran since)
    int64_t tree_visits = 0;      // the most root visits any of those trees can hold by now
    bool ply_trees = false;       // the trees are the previous self-play ply's (cleared by oaz_selfplay_reset and any search)
    unsigned long long out_read = 0;  // samples already handed out
    bool selfplay_ready = false;
    uint64_t quota = 0;
    // events (after the buffers: destroyed before them)
    Event ev_join, ev_part[kMaxParts];   // (ev_part[0] is never made: part 0 runs on `stream`)
    Event ev_ready[2];
    Event ev_consumed[2][kMaxParts];     // noise ring slot done with, per game part
    // timing
    bool timing = false;
    int timing_every = 1;     // time the kernels of every N-th simulation step (events cost ~2 % each)
    bool timing_skip = false; // run_sims: this simulation step is not sampled
    std::vector<TimedLaunch> pending;
    std::vector<Event> pool;
    oaz_kernel_times times{};
};

static TreeView tree_view(oaz_engine* e, uint32_t G) {
    TreeView t;
    t.nodes = e->nodes;
    t.n_nodes = e->n_nodes;
    t.path = e->path;
    t.depth = e->depth;
    t.leaf = e->leaf;
    t.leaf_state = e->leaf_state;
    t.stats = e->stats;
    t.sqrt_tab = e->sqrt_tab;
    t.need = e->need;
    t.slot = e->slot;
    t.cstate = e->cstate;
    t.bcnt = e->bcnt;
    t.cap = e->cap;
    t.pathcap = e->pathcap;
    t.G = G;
    return t;
}

static SlotView slot_view(oaz_engine* e) {
    SlotView s;
    s.root = e->root;
    s.ply = e->ply;
    s.seq = e->seq;
    s.game_id = e->game_id;
    s.active = e->active;
    s.hist = e->hist;
    s.out = e->out;
    s.out_count = e->out_count;
    s.fin = e->fin;
    s.fin_pos = e->fin_pos;
    s.hcap = e->hcap;
    s.out_cap = e->out_cap;
    s.max_plies = e->cfg.max_plies;
    s.fixed_deck = e->cfg.fixed_deck;
    memcpy(s.deck, e->cfg.deck, 5);
    s.seed = e->cfg.seed;
    s.G = e->G;
    s.world = (uint32_t)(e->cfg.world > 0 ? e->cfg.world : 1);
    s.rank = (uint32_t)e->cfg.rank;
    s.quota = e->quota;
    s.stagger = e->quota ? 0u : (uint32_t)(e->cfg.stagger > 0 ? e->cfg.stagger : 0);
    return s;
}

static CapView cap_view(const oaz_engine* e) {
    CapView c;
    c.full = e->pc_flags;
    c.fast = e->pc_flags + e->G;
    c.fullm = e->pc_flags + 2 * (size_t)e->G;
    c.nrec = e->pc_nrec;
    c.cnt = e->pc_cnt;
    c.P = e->pc_share;
    return c;
}

static SearchParams search_params(const oaz_engine* e) {
    SearchParams p;
    p.c_puct = e->cfg.c_puct;
    p.alpha = e->cfg.dirichlet_alpha;
    p.eps = e->cfg.dirichlet_eps;
    p.seed = e->cfg.seed;
    p.train_noise = e->cfg.train_noise;
    return p;
}

// A timing event from the pool, or a new one (one that could not be made fails its first hipEventRecord).
static Event ev_get(oaz_engine* e) {
    if (e->pool.empty()) {
        Event ev;
        (void)ev.create(hipEventDefault);
        return ev;
    }
    Event ev = std::move(e->pool.back());
    e->pool.pop_back();
    return ev;
}

// Run a launch, bracketed by events on the engine stream when timing is on.
#ifndef OAZ_NOISE_CHUNK  // 16: C3 +0.3 % over 8 in a 4-round same-box A/B (50: +0.4 %, 3x the ring); DESIGN.md perf log
#define OAZ_NOISE_CHUNK 16
#endif
static constexpr uint32_t kNoiseChunk = OAZ_NOISE_CHUNK;  // simulations of root noise produced per launch
static uint32_t noise_chunk_for(const oaz_engine* e);  // after search_path

static void accumulate(oaz_engine* e, const TimedLaunch& p, float ms) {
    oaz_kernel_times& t = e->times;
    const struct { double* ms; uint64_t* n; } of[K_COUNT] = {
        {&t.select_ms, &t.select_n},     {&t.nn_ms, &t.nn_n},       {&t.expand_ms, &t.expand_n},
        {&t.finalize_ms, &t.finalize_n}, {&t.noise_ms, &t.noise_n}, {&t.compact_ms, &t.compact_n},
        {&t.backup_select_ms, &t.backup_select_n}};
    *of[p.kind].ms += ms;
    *of[p.kind].n += 1;
    if (p.kind == K_NN) t.nn_samples += p.samples;
}

// Resolve the recorded event pairs: per-kind sums, and the NN's busy time = the length of the union
// of its launches' intervals (with game parts on several streams the NN launches of a simulation
// step overlap each other; the union is the time during which any of them ran).
static int resolve_pending(oaz_engine* e) {
    std::vector<std::pair<float, float>> nn;
    hipEvent_t ref = e->pending.empty() ? nullptr : e->pending.front().a;
    for (auto& p : e->pending) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        accumulate(e, p, ms);
        if (p.kind == K_NN) {
            float t0 = 0.f;
            HIP_TRY(hipEventElapsedTime(&t0, ref, p.a));
            nn.emplace_back(t0, t0 + ms);
        }
    }
    std::sort(nn.begin(), nn.end());
    for (size_t i = 0; i < nn.size();) {
        float lo = nn[i].first, hi = nn[i].second;
        size_t j = i + 1;
        for (; j < nn.size() && nn[j].first <= hi; ++j) hi = std::max(hi, nn[j].second);
        e->times.nn_busy_ms += hi - lo;
        e->times.nn_busy_n += 1;
        i = j;
    }
    for (auto& p : e->pending) {
        e->pool.push_back(std::move(p.a));
        e->pool.push_back(std::move(p.b));
    }
    e->pending.clear();
    return 0;
}

// Waits for all the engine's streams.
static int sync_streams(oaz_engine* e) {
    HIP_TRY(e->stream.sync());
    HIP_TRY(e->stream2.sync());
    for (auto& s3 : e->stream3) HIP_TRY(s3.sync());
    return 0;
}

static int resolve_timing(oaz_engine* e) {
    if (int rc = sync_streams(e)) return rc;
    return resolve_pending(e);
}

template <class F>
static int timed(oaz_engine* e, LaunchKind kind, uint32_t samples, F&& launch, hipStream_t st = nullptr) {
    if (!st) st = e->stream;
    if (!e->timing || e->timing_skip) {
        HIP_TRY(launch());
        return 0;
    }
    TimedLaunch t{kind, ev_get(e), ev_get(e), samples};
    HIP_TRY(hipEventRecord(t.a, st));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(t.b, st));
    e->pending.push_back(std::move(t));
    if (e->pending.size() > 4096) return resolve_timing(e);  // resolve periodically to bound the pool
    return 0;
}

// The argument checks of oaz_create.
// Root visits a tree is sized for: the playouts of one search, or with tree reuse its capacity R >= sims.
static uint32_t tree_visits_cap(const oaz_config* cfg) {
    return (uint32_t)(cfg->reuse_visits > 0 ? cfg->reuse_visits : cfg->sims);
}
constexpr int kMaxLeafBatch = 16;  // oaz_config.leaf_batch: the leaves of a round are one network tile
constexpr int32_t kMaxReuseVisits = 1 << 20;  // 1 + R * OAZ_MAX_MOVES nodes fit 32-bit node indices with room

static int create_check(const oaz_config* cfg, int device) {
    if (!cfg) return oaz_set_err(OAZ_ERR_ARG, "create: null config");
    if (cfg->channels != 64 || cfg->in_planes != 21)
        return oaz_set_err(OAZ_ERR_ARG, "create: only channels=64, in_planes=21 are supported");
    if (cfg->blocks < 0 || cfg->blocks > 64 || cfg->sims < 1 || cfg->sims > 65535 || cfg->games < 1 ||
        cfg->max_plies < 0 || cfg->max_plies > 100000 || cfg->compact < 0 || cfg->compact > 2 || cfg->search_time_ns < 0 ||
        cfg->step_kernels < 0 || cfg->step_kernels > 1 || cfg->world < 0 || cfg->rank < 0 ||
        cfg->rank >= (cfg->world > 0 ? cfg->world : 1) ||
        cfg->reuse_visits < 0 || cfg->reuse_visits > kMaxReuseVisits ||
        (uint64_t)cfg->games * ((uint64_t)tree_visits_cap(cfg) + 1) >= (1ull << 32) ||  // 32-bit path offsets (k_select_seg)
        (uint64_t)cfg->games * kNoiseStride * sizeof(noise_t) >= (1ull << 31) ||  // 32-bit noise offsets (root_noise_pairs)
        (cfg->parts != 0 && cfg->parts != 1 && cfg->parts != 2 && cfg->parts != 4))
        return oaz_set_err(OAZ_ERR_ARG, "create: config out of range");
    if (cfg->reuse_visits > 0 && cfg->reuse_visits < cfg->sims)
        return oaz_set_err(OAZ_ERR_ARG, "create: reuse_visits=%d < sims=%d (a tree must hold one search)", cfg->reuse_visits,
                           cfg->sims);
    if (cfg->reuse_visits > 0 && !launch_selfplay_rebase)
        return oaz_set_err(OAZ_ERR_ARG, "create: reuse_visits > 0 in a build without the tree reuse kernels");
    if (cfg->temperature_plies > 0 && !launch_selfplay_move_temp)
        return oaz_set_err(OAZ_ERR_ARG, "create: temperature_plies > 0 in a build without the temperature kernel");
    if (cfg->precision != OAZ_FP32 && cfg->precision != OAZ_BF16 && cfg->precision != OAZ_FP32_SPLIT &&
        cfg->precision != OAZ_FP32_SPLIT16)
        return oaz_set_err(OAZ_ERR_ARG, "create: precision must be OAZ_FP32, OAZ_BF16, OAZ_FP32_SPLIT or OAZ_FP32_SPLIT16");
    if (cfg->leaf_batch > kMaxLeafBatch)
        return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch=%d > %d (one 16-position tile)", cfg->leaf_batch, kMaxLeafBatch);
    if (cfg->leaf_batch > 0) {  // the combinations that could never run the leaf-parallel search: no other algorithm
        if (!launch_search_par)
            return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch > 0 in a build without the leaf-parallel search kernel");
        if (cfg->step_kernels == 1)
            return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch > 0 needs step_kernels = 0 (it is a one-launch search)");
        if (cfg->compact != 0) return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch > 0 needs compact = 0");
        if (cfg->evaluator != OAZ_EVAL_HASH && cfg->precision != OAZ_FP32_SPLIT16)
            return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch > 0 needs the fp16x3 network (OAZ_FP32_SPLIT16) or HASH");
        if (cfg->reuse_visits > 0)
            return oaz_set_err(OAZ_ERR_ARG, "create: leaf_batch > 0 and reuse_visits > 0 (tree reuse) do not combine");
    }
    return oaz_check_device("create", device);
}

// The device side of oaz_create: streams, events, buffers and their first contents. On an error the engine is
// partly built; oaz_destroy takes it as it is (a member not made yet holds nothing).
static int engine_init(oaz_engine* e) {
    const oaz_config* cfg = &e->cfg;
    OAZ_ON_DEVICE(e->device);  // the caller's current device is restored on return
    if (e->stream.create() || e->stream2.create() || e->ev_join.create()) return OAZ_ERR_HIP;
    for (int i = 0; i < kMaxParts - 1; ++i)
        if (e->stream3[i].create() || e->ev_part[i + 1].create()) return OAZ_ERR_HIP;
    for (int i = 0; i < 2; ++i) {
        if (e->ev_ready[i].create()) return OAZ_ERR_HIP;
        for (auto& ev : e->ev_consumed[i])
            if (ev.create()) return OAZ_ERR_HIP;
    }
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || e->cus < 1)
        e->cus = 256;
    if (hipDeviceGetAttribute(&e->wall_khz, hipDeviceAttributeWallClockRate, e->device) != hipSuccess) e->wall_khz = 0;
    const size_t G = e->G;
    e->noise_chunk = noise_chunk_for(e);
    if (e->nodes.alloc(G * e->cap) || e->n_nodes.alloc(G) || e->path.alloc(G * e->pathcap) || e->depth.alloc(G) ||
        e->leaf.alloc(G) || e->leaf_state.alloc(G) || e->stats.alloc(G * GS_COUNT) || e->stats_sum.alloc(GS_COUNT) ||
        e->sqrt_tab.alloc((size_t)tree_visits_cap(cfg) + 2) || e->policy.alloc(G * 50) || e->value.alloc(G) || e->need.alloc(G) ||
        e->slot.alloc(G) || e->cstate.alloc(G + 16) || e->bcnt.alloc((size_t)buckets_of((uint32_t)G) + kMaxParts) ||
        e->weights.alloc(nn_device_floats(cfg->blocks, cfg->precision)) || e->s_roots.alloc(G) || e->s_move.alloc(G) ||
        e->s_pi.alloc(G * 50) || e->s_rootv.alloc(G) || e->s_rootp.alloc(G * 50) || e->s_ply.alloc(G) ||
        e->root.alloc(G) || e->ply.alloc(G) || e->seq.alloc(G) || e->game_id.alloc(G) || e->active.alloc(G) ||
        e->hist.alloc(G * e->hcap) || e->out.alloc(e->out_cap) || e->out_count.alloc(1) || e->nn_fallback.alloc(1) ||
        e->deadline.alloc(1) || e->sims_run.alloc(G) || e->fin.alloc(G) || e->fin_pos.alloc(G) ||
        (cfg->train_noise && e->noise.alloc(2 * (size_t)e->noise_chunk * G * kNoiseStride)))
        return OAZ_ERR_HIP;  // (alloc's HIP_TRY recorded the call and the HIP error)
    if (cfg->reuse_visits > 0 &&
        (e->adv_moves.alloc(G) || e->adv_codes.alloc(G) || e->adv_kept.alloc(G) || e->reuse_cnt.alloc(4)))
        return OAZ_ERR_HIP;
    if (cfg->temperature_plies > 0 && e->temp_cnt.alloc(2)) return OAZ_ERR_HIP;
    if (const size_t L = cfg->leaf_batch) {
        if (e->par_path.alloc(G * L * e->pathcap) || e->par_depth.alloc(G * L) || e->par_leaf.alloc(G * L) ||
            e->par_state.alloc(G * kMaxLeafBatch) || e->par_policy.alloc(G * kMaxLeafBatch * 50) ||
            e->par_value.alloc(G * kMaxLeafBatch) || e->par_stats.alloc(G * 3))
            return OAZ_ERR_HIP;
    }
    // sqrt((double)n) from the host libm (IEEE correctly rounded), so device PUCT = oracle PUCT
    std::vector<double> tab((size_t)tree_visits_cap(cfg) + 2);
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = sqrt((double)i);
    // on the engine's own stream, waited for: its streams do not synchronise with the null stream, a null-stream
    // hipMemset returns before it ran and a pageable hipMemcpy before its DMA landed, so the first kernels could
    // otherwise read these buffers early (seen with several engines created concurrently on one GPU)
    hipStream_t s0 = e->stream;
    HIP_TRY(hipMemcpyAsync(e->sqrt_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s0));
    HIP_TRY(hipMemsetAsync(e->stats, 0, G * GS_COUNT * sizeof(uint64_t), s0));
    HIP_TRY(hipMemsetAsync(e->out_count, 0, sizeof(unsigned long long), s0));
    HIP_TRY(hipMemsetAsync(e->nn_fallback, 0, sizeof(unsigned long long), s0));
    HIP_TRY(hipMemsetAsync(e->active, 0, G, s0));
    HIP_TRY(hipMemsetAsync(e->need, 0, G, s0));
    HIP_TRY(hipMemsetAsync(e->slot, 0, G * sizeof(uint32_t), s0));
    HIP_TRY(hipMemsetAsync(e->cstate, 0, (G + 16) * sizeof(oaz_state), s0));
    if (e->reuse_cnt) HIP_TRY(hipMemsetAsync(e->reuse_cnt, 0, 4 * sizeof(uint64_t), s0));
    if (e->temp_cnt) HIP_TRY(hipMemsetAsync(e->temp_cnt, 0, 2 * sizeof(uint64_t), s0));
    if (e->par_state) {
        HIP_TRY(hipMemsetAsync(e->par_state, 0, G * kMaxLeafBatch * sizeof(oaz_state), s0));
        HIP_TRY(hipMemsetAsync(e->par_stats, 0, G * 3 * sizeof(uint64_t), s0));
    }
    HIP_TRY(hipStreamSynchronize(s0));
    if (cfg->evaluator == OAZ_EVAL_NN) {  // random-init weights until oaz_load_weights
        std::vector<float> w(oaz_weight_count(cfg->blocks, 64, 21));
        if (int rc = oaz_random_weights(0, cfg->blocks, w.data(), w.size())) return rc;
        if (int rc = oaz_load_weights(e, w.data(), w.size())) return rc;
    }
    return 0;
}

extern "C" oaz_engine* oaz_create(const oaz_config* cfg, int device) {
    if (create_check(cfg, device)) return nullptr;
    oaz_engine* e = new oaz_engine();
    e->cfg = *cfg;
    e->device = device;
    e->G = (uint32_t)cfg->games;
    e->sims_cap = cfg->sims;
    e->cap = 1u + tree_visits_cap(cfg) * OAZ_MAX_MOVES;  // each playout expands <= 1 node of <= 40 children
    e->pathcap = tree_visits_cap(cfg) + 1;               // depth grows by <= 1 per playout
    e->hcap = (uint32_t)cfg->max_plies + 2;             // train.rs:74-79 cut after max_plies+2 plies
    e->out_cap = cfg->sample_capacity > 0 ? (uint32_t)cfg->sample_capacity : e->G * 64u;
    if (engine_init(e)) {  // the one failure exit: the partly built engine goes, the error text stays
        const std::string msg = g_err;
        oaz_destroy(e);
        g_err = msg;
        return nullptr;
    }
    return e;
}

// On the engine's device: wait for its streams, then `delete` destroys the members (events, buffers, streams
// last: the declaration order of oaz_engine), the timing events in `pending` and `pool` among them.
extern "C" void oaz_destroy(oaz_engine* e) {
    if (!e) return;
    DeviceScope dev_scope_(e->device);
    (void)e->stream.sync();
    (void)e->stream2.sync();
    for (auto& s3 : e->stream3) (void)s3.sync();
    delete e;
}

extern "C" int oaz_set_search_params(oaz_engine* e, int sims, double c_puct, int train_noise) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "set_search_params: null");
    if (sims < 1 || sims > e->sims_cap)
        return oaz_set_err(OAZ_ERR_ARG, "set_search_params: sims %d outside [1, %d] (the creation budget)", sims,
                           e->sims_cap);
    if (!(c_puct >= 0.0) || !std::isfinite(c_puct)) return oaz_set_err(OAZ_ERR_ARG, "set_search_params: bad c_puct");
    if (train_noise && !e->noise) {  // the engine was made without root noise: its ring comes now
        OAZ_ON_DEVICE(e->device);
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (int rc = e->noise.alloc(2 * (size_t)e->noise_chunk * e->G * kNoiseStride)) return rc;
    }
    e->cfg.sims = sims;
    e->cfg.c_puct = c_puct;
    e->cfg.train_noise = train_noise ? 1 : 0;
    return 0;
}

extern "C" int oaz_set_search_time(oaz_engine* e, int64_t search_time_ns) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "set_search_time: null");
    if (search_time_ns < 0) return oaz_set_err(OAZ_ERR_ARG, "set_search_time: negative budget");
    e->cfg.search_time_ns = search_time_ns;
    return 0;
}

// The device-budgeted searches leave each game's count on the device; read them once.
static int fetch_sims_run(oaz_engine* e) {
    LastSearch& L = e->last;
    if (!L.on_device) return 0;
    OAZ_ON_DEVICE(e->device);
    std::vector<uint32_t> n(L.G);
    if (L.G) {
        HIP_TRY(hipMemcpyAsync(n.data(), e->sims_run, (size_t)L.G * 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    L.sims = n.empty() ? 0 : *std::max_element(n.begin(), n.end());
    L.on_device = false;
    L.per_game = std::move(n);
    return 0;
}

extern "C" int oaz_last_sims(oaz_engine* e, int* sims) {
    if (!e || !sims) return oaz_set_err(OAZ_ERR_ARG, "last_sims: null");
    if (int rc = fetch_sims_run(e)) return rc;
    *sims = (int)e->last.sims;
    return 0;
}

extern "C" int oaz_search_playouts(oaz_engine* e, int* out, int G) {
    if (!e || (!out && G > 0) || G < 0) return oaz_set_err(OAZ_ERR_ARG, "search_playouts: bad arguments");
    if ((uint32_t)G > e->last.G)
        return oaz_set_err(OAZ_ERR_ARG, "search_playouts: G=%d > %u games in the last search", G, e->last.G);
    if (int rc = fetch_sims_run(e)) return rc;
    for (int g = 0; g < G; ++g) out[g] = (int)(e->last.per_game.empty() ? e->last.sims : e->last.per_game[(size_t)g]);
    return 0;
}

extern "C" int oaz_search_leaf_batch_stats(oaz_engine* e, uint64_t out[3]) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "search_leaf_batch_stats: null");
    out[0] = out[1] = out[2] = 0;
    if (e->cfg.leaf_batch == 0 || e->par_G == 0) return 0;
    OAZ_ON_DEVICE(e->device);
    std::vector<uint64_t> v((size_t)e->par_G * 3);
    HIP_TRY(hipMemcpyAsync(v.data(), e->par_stats, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < v.size(); ++i) out[i % 3] += v[i];
    return 0;
}

extern "C" int oaz_get_config(const oaz_engine* e, oaz_config* out) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "get_config: null");
    *out = e->cfg;
    return 0;
}

extern "C" int oaz_load_weights(oaz_engine* e, const float* blob, size_t n) {
    if (!e || !blob) return oaz_set_err(OAZ_ERR_ARG, "load_weights: null");
    const size_t need = oaz_weight_count(e->cfg.blocks, 64, 21);
    if (n != need)  // the reference silently keeps random weights on a bad file (Q13); we refuse
        return oaz_set_err(OAZ_ERR_WEIGHTS, "load_weights: got %zu floats, need %zu for %d blocks", n, need,
                       e->cfg.blocks);
    std::vector<float> packed;
    if (int rc = oaz_pack_weights(blob, n, e->cfg.blocks, e->cfg.precision, packed))
        return oaz_set_err(OAZ_ERR_STATE, "load_weights: pack failed (code %d)", rc);
    OAZ_ON_DEVICE(e->device);
    HIP_TRY(hipMemcpyAsync(e->weights, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_weights = true;
    return 0;
}

extern "C" int oaz_sync(oaz_engine* e) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "sync: null");
    OAZ_ON_DEVICE(e->device);
    return sync_streams(e);
}

extern "C" int oaz_set_timing(oaz_engine* e, int enable) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "set_timing: null");
    if (enable < 0) return oaz_set_err(OAZ_ERR_ARG, "set_timing: enable=%d < 0", enable);
    e->timing = enable != 0;
    e->timing_every = enable > 1 ? enable : 1;
    return 0;
}

extern "C" int oaz_kernel_times_get(oaz_engine* e, oaz_kernel_times* out) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "kernel_times: null");
    if (int rc = resolve_timing(e)) return rc;
    *out = e->times;
    return 0;
}

extern "C" int oaz_kernel_times_reset(oaz_engine* e) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "kernel_times_reset: null");
    if (int rc = resolve_timing(e)) return rc;
    memset(&e->times, 0, sizeof(e->times));
    return 0;
}

static NNView nn_view(const oaz_engine* e, const TileMap* tm) {
    NNView w;
    w.blob = e->weights;
    w.blocks = e->cfg.blocks;
    w.precision = e->cfg.precision;
    w.x6_variant = 0;
#if OAZ_AB  // A/B build only: the diagnostic builds of k_nn_h3 by environment variable
    if (const char* xv = getenv("OAZ_NN_X6_V")) w.x6_variant = atoi(xv);
#endif
    w.blob_x6 = e->cfg.precision == OAZ_FP32_SPLIT16 ? e->weights + nn_packed_floats(e->cfg.blocks, OAZ_FP32_SPLIT16)
                                                     : nullptr;
    w.fallback = e->nn_fallback;
    w.tm = tm ? *tm : TileMap{nullptr, 0, 0};
    // k_nn_h3s (one position per workgroup) while the launch fits one round of workgroups on the CUs;
    // k_nn_h3 (16 per workgroup) above. The two give bit-identical outputs.
    w.small_max = e->cus;
#if OAZ_AB  // A/B build only: OAZ_NN_SMALL_MAX=n overrides
    if (const char* v = getenv("OAZ_NN_SMALL_MAX")) w.small_max = atoi(v);
#endif
    return w;
}

// B positions d_states[0, B) -> rows [0, B); with tm (compacted leaves, run_sims) the rows of the
// bucket tiles (the HASH evaluator simply evaluates every row below B).
static int evaluate(oaz_engine* e, const oaz_state* d_states, uint32_t B, float* d_pol, float* d_val,
                    hipStream_t st = nullptr, const TileMap* tm = nullptr) {
    if (!st) st = e->stream;
    const uint32_t counted = tm ? 0u : B;  // compacted: the count is on the device (GS_EVALS)
    if (e->cfg.evaluator == OAZ_EVAL_HASH)
        return timed(e, K_NN, counted, [&] { return launch_hash_eval(d_states, (int)B, d_pol, d_val, st); }, st);
    const NNView w = nn_view(e, tm);
    return timed(e, K_NN, counted, [&] { return launch_nn_forward(w, d_states, (int)B, d_pol, d_val, st); }, st);
}

extern "C" int oaz_nn_fallbacks(oaz_engine* e, uint64_t* tiles) {
    if (!e || !tiles) return oaz_set_err(OAZ_ERR_ARG, "nn_fallbacks: null");
    OAZ_ON_DEVICE(e->device);
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, e->nn_fallback, sizeof(n), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *tiles = (uint64_t)n;
    return 0;
}

extern "C" int oaz_nn_forward(oaz_engine* e, const oaz_state* s, int B, float* policy, float* value) {
    if (!e || !s || B < 0) return oaz_set_err(OAZ_ERR_ARG, "nn_forward: bad arguments");
    if ((uint32_t)B > e->G) return oaz_set_err(OAZ_ERR_CAPACITY, "nn_forward: B=%d > games=%u", B, e->G);
    if (B == 0) return 0;
    OAZ_ON_DEVICE(e->device);
    HIP_TRY(hipMemcpyAsync(e->s_roots, s, (size_t)B * sizeof(oaz_state), hipMemcpyHostToDevice, e->stream));
    if (int rc = evaluate(e, e->s_roots, (uint32_t)B, e->s_rootp, e->s_rootv)) return rc;
    if (policy) HIP_TRY(hipMemcpyAsync(policy, e->s_rootp, (size_t)B * 50 * 4, hipMemcpyDeviceToHost, e->stream));
    if (value) HIP_TRY(hipMemcpyAsync(value, e->s_rootv, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// ---- the search driver (run_sims) -------------------------------------------------------------------
// Leaf compaction (oaz_config.compact; off by default: every playout evaluates its leaf, Q2) pays
// when it can remove whole rounds of NN workgroups (one 16-position tile per
// CU at a time): at C3 the ~8.7 % won leaves are 1.4 of 16 rounds. Below 12 rounds (G < 12 * 16 *
// CUs, e.g. C2's 4096 games = one round) it would only add its own launch, so the leaves are then
// evaluated in place.
static bool compact_leaves(const oaz_engine* e, uint32_t G) {
    return e->cfg.compact == 1 || (e->cfg.compact == 2 && G >= 12u * 16u * (uint32_t)e->cus);
}

// How a search of G games runs. Both one-launch searches (oaz_search_lat.hip) need the segmented tree kernels
// they are built from, every leaf evaluated in place, and an evaluator they contain (HASH, or the fp16x3
// network); everything they depend on is fixed at creation except G and the noise.
//   LAT    k_search_lat: a workgroup per game runs all its simulations in one launch, when the per-step loop
//          would launch one NN workgroup per game anyway and nothing needs a second stream (the root noise)
//          between steps;
//   GRP    k_search_grp: 16 games per workgroup, up to one round of workgroups, one launch per root-noise
//          chunk (any G below a qualifying engine's qualifies as well);
//   STEPS  the per-simulation-step launches; always so for a search that goes on with kept trees (tree reuse).
//   PAR    k_search_par: an engine with leaf_batch > 0, every search it accepts (par_search_check refuses the
//          others; create_check the configurations that never could).
enum SearchPath { PATH_LAT, PATH_GRP, PATH_STEPS, PATH_PAR };
static SearchPath search_path(const oaz_engine* e, uint32_t G, bool noise, bool kept_trees = false) {
    if (e->cfg.leaf_batch > 0) return PATH_PAR;
    const bool one_launch = !kept_trees && e->cfg.step_kernels == 0 && !compact_leaves(e, G) &&
                            (e->cfg.evaluator == OAZ_EVAL_HASH || e->cfg.precision == OAZ_FP32_SPLIT16) &&
                            tree_seg_kernels();
    if (!one_launch) return PATH_STEPS;
    if (!noise && G <= (uint32_t)e->cus) return PATH_LAT;
    return (G + 15) / 16 <= (uint32_t)e->cus ? PATH_GRP : PATH_STEPS;
}

// Simulations per root-noise ring slot. An engine whose searches run as k_search_grp: every chunk is one
// launch, and the noise launch of the next chunk cannot overlap it (the search holds every CU), so a chunk of
// up to 512 simulations (a C2 ply in one launch and one noise launch: 46.6-47.1 -> 49.5-50.0 M sims/s;
// DESIGN.md section 8) at a 16-simulation minimum. kNoiseChunk (16) for the per-step launches, where the
// noise overlaps the network and the first select waits for only 16 simulations' draws. Ring: 2 x chunk x
// G x 80 floats (<= 1.3 GB at 4 096 games).
static uint32_t noise_chunk_for(const oaz_engine* e) {
    // (an engine with tree reuse goes on with kept trees, which run the per-step launches at every size)
    if (search_path(e, e->G, true, e->cfg.reuse_visits > 0) != PATH_GRP) return kNoiseChunk;
    return std::max(kNoiseChunk, std::min((uint32_t)e->sims_cap, 512u));
}

// Game parts of the per-step loop (oaz_config.parts; 0 = auto: two from kAutoParts games; the overlap of
// one part's tree kernels and NN tail with the other's launches measured +3-4 % on C2, C3, C5).
constexpr uint32_t kAutoParts = 2048;
static int game_parts(const oaz_engine* e, uint32_t G) {
    int p = e->cfg.parts ? e->cfg.parts : (G >= kAutoParts ? 2 : 1);
    // every part non-empty: part h starts at h * ceil(G / p), so the last one needs (p - 1) * ceil(G / p) < G
    // (G = 5, p = 4 would give parts of 2, 2, 1 and an empty fourth)
    while (p > 1 && (uint32_t)(p - 1) * ((G + (uint32_t)p - 1) / (uint32_t)p) >= G) p /= 2;
    return p;
}

// The trees of games [g0, g0 + n) as a view of their own: every per-game array offset by g0, the
// part's compaction buckets from bucket counter b0 (its compacted rows start at g0; the NN's row loads
// are clamped to the part's own n rows by the TileMap cap, sim_step).
static TreeView slice_view(const TreeView& t, uint32_t g0, uint32_t n, int b0) {
    TreeView v = t;
    v.nodes = t.nodes + (size_t)g0 * t.cap;
    v.n_nodes = t.n_nodes + g0;
    v.path = t.path + (size_t)g0 * t.pathcap;
    v.depth = t.depth + g0;
    v.leaf = t.leaf + g0;
    v.leaf_state = t.leaf_state + g0;
    v.stats = t.stats + (size_t)g0 * GS_COUNT;
    if (t.need) v.need = t.need + g0;
    if (t.slot) v.slot = t.slot + g0;
    v.cstate = t.cstate + g0;
    v.bcnt = t.bcnt + b0;
    v.G = n;
    return v;
}

// One run_sims call: the trees of all its games, the positions searched and what every launch shares.
struct Search {
    TreeView t;              // with the compaction arrays, or none (rows = game ids)
    const oaz_state* roots;
    const uint8_t* active;   // null in search mode,
    const uint64_t* gids;    // as are the game ids
    const uint32_t* plies;
    SearchParams prm;
    uint32_t sims;
    bool noise;
    const NNView* net;       // the one-launch searches' network (null: the HASH evaluator)
    uint64_t* deadline;      // Q7 on the device (the one-launch searches): both null without a budget
    uint32_t* sims_run;
};

// The games in n parts, each on its own stream: one part's tree kernels, leaf compaction and NN
// tail run in the gaps of the others' launches (the NN holds a whole CU per workgroup, so the
// tree kernels cannot share a CU with it, only fill the CUs it leaves idle). The parts meet only
// through the root-noise ring. Part h holds games [g0, g0 + t.G): ceil(G / n) each, the last one the rest.
struct Parts {
    struct Part {
        TreeView t;
        uint32_t g0;
        hipStream_t st;
        const oaz_state* roots;
        const uint8_t* active;
        float *pol, *val;  // the part's rows of the evaluations
    };
    oaz_engine* e;
    int n;
    Part part[kMaxParts];
    Parts(oaz_engine* e, const Search& S, int n) : e(e), n(n) {
        const uint32_t G = S.t.G, each = (G + (uint32_t)n - 1) / (uint32_t)n;
        int b0 = 0;  // a part's compaction bucket counters follow the previous parts'
        for (int h = 0; h < n; ++h) {
            const uint32_t g0 = (uint32_t)h * each, cnt = std::min(each, G - g0);
            const hipStream_t st = h ? e->stream3[h - 1] : e->stream;
            part[h] = {slice_view(S.t, g0, cnt, b0), g0, st, S.roots + g0,
                       S.active ? S.active + g0 : nullptr, e->policy + (size_t)g0 * 50, e->value + g0};
            b0 += buckets_of(cnt);
        }
    }
    int fork() const {  // the other parts' streams start after prior work on the engine stream
        if (n > 1) HIP_TRY(hipEventRecord(e->ev_join, e->stream));
        for (int h = 1; h < n; ++h) HIP_TRY(hipStreamWaitEvent(part[h].st, e->ev_join, 0));
        return 0;
    }
    int join() const {  // the engine stream waits for the other parts' streams
        for (int h = 1; h < n; ++h) {
            HIP_TRY(hipEventRecord(e->ev_part[h], part[h].st));
            HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_part[h], 0));
        }
        return 0;
    }
};

// The root-noise ring of one search: e->noise holds two slots of `chunk` simulations' draws for the search's
// games, chunk c in slot c & 1. k_root_noise fills chunk c + 1 on stream2 while the parts run chunk c, and
// chunk c + 2 may overwrite chunk c's slot only after every part has released it; the events below carry
// that rule, so the callers name chunks and simulations, never slots. Without root noise every operation
// does nothing and at() is null.
struct NoiseRing {
    oaz_engine* e;
    const Search& S;
    const Parts& P;
    uint32_t chunk;  // simulations per slot (e->noise_chunk)
    noise_t* slot(uint32_t c) const { return e->noise + (c & 1) * ((size_t)chunk * S.t.G * kNoiseStride); }
    const noise_t* at(uint32_t s, uint32_t g0) const {  // simulation s's draws for the games from g0 on
        return S.noise ? slot(s / chunk) + ((size_t)(s % chunk) * S.t.G + g0) * kNoiseStride : nullptr;
    }
    // k_root_noise for chunk c (if the search has one) on stream2: chunk 0 after prior work on the engine
    // stream, chunk c >= 2 after every part released chunk c - 2
    int produce(uint32_t c) const {
        if (!S.noise || c * chunk >= S.sims) return 0;
        if (c == 0) {
            HIP_TRY(hipEventRecord(e->ev_consumed[0][0], e->stream));
            HIP_TRY(hipStreamWaitEvent(e->stream2, e->ev_consumed[0][0], 0));
        } else if (c >= 2) {
            for (int h = 0; h < P.n; ++h) HIP_TRY(hipStreamWaitEvent(e->stream2, e->ev_consumed[c & 1][h], 0));
        }
        e->timing_skip = false;  // every noise launch is timed (once per chunk)
        const uint32_t s0 = c * chunk, n = std::min(S.sims - s0, chunk);
        if (int rc = timed(e, K_NOISE, S.t.G * n, [&] {
                return launch_root_noise(S.roots, S.active, S.gids, S.plies, S.prm, S.t.G, s0, n, slot(c), e->stream2);
            }, e->stream2))
            return rc;
        HIP_TRY(hipEventRecord(e->ev_ready[c & 1], e->stream2));
        return 0;
    }
    int wait(uint32_t c) const {  // every part's stream waits for chunk c's draws
        for (int h = 0; S.noise && h < P.n; ++h) HIP_TRY(hipStreamWaitEvent(P.part[h].st, e->ev_ready[c & 1], 0));
        return 0;
    }
    // every part is done with chunk c at this point of its stream (no join: a part may run a chunk ahead)
    int release(uint32_t c) const {
        for (int h = 0; S.noise && h < P.n; ++h) HIP_TRY(hipEventRecord(e->ev_consumed[c & 1][h], P.part[h].st));
        return 0;
    }
};

// Q7: a search's budget runs from the start of the search call (every run_sims follows one of these), as the
// reference's Instant is taken at the top of search() (mcts_arena.rs:75-78): the host clock now (the per-step
// loop's reads) and, on the device, the deadline = the device clock when k_deadline_start runs + the budget,
// armed before this search's first upload or reset on the engine stream (the one-launch searches' reads),
// so the roots upload and the tree reset count against the budget on both paths. Work queued on the stream
// by earlier calls (asynchronous self-play plies) is not part of this search.
static int begin_budget(oaz_engine* e) {
    e->t_search0 = 0.0;
    if (e->cfg.search_time_ns <= 0) return 0;
    e->t_search0 = now_ns();
    if (e->wall_khz <= 0) return 0;  // (no device clock: only the one-launch searches need it, arm_device_budget)
    HIP_TRY(launch_deadline_start(e->deadline, oaz_budget_ticks(e->cfg.search_time_ns, e->wall_khz, 1.8e19), e->stream));
    return 0;
}

// Q7 (opt-in, oaz_config.search_time_ns): the reference's loop runs playouts while
// `playouts < max_playouts && elapsed < search_time` (mcts_arena.rs:78). The one-launch searches
// (k_search_lat, k_search_grp: the Agent / arena sizes) read the device clock before every simulation
// and each workgroup stops on its own (oaz_search_playouts: each game's count, >= 1) at begin_budget's
// deadline; every game's count starts at 0.
static int arm_device_budget(oaz_engine* e, uint32_t G) {
    if (e->cfg.search_time_ns <= 0) return 0;
    if (e->wall_khz <= 0) return oaz_set_err(OAZ_ERR_HIP, "search_time: the device reports no wall clock rate");
    HIP_TRY(hipMemsetAsync(e->sims_run, 0, (size_t)G * 4, e->stream));
    e->last.on_device = true;
    return 0;
}

// k_search_lat: the whole search in one launch, the last simulation's expand/backup included.
static int search_lat(oaz_engine* e, const Search& S) {
    e->times.parts = 1;
    if (int rc = timed(e, K_BACKUP_SELECT, S.t.G, [&] {
            return launch_search_lat(S.t, S.roots, S.active, S.prm, (int)S.sims, S.net, e->policy, e->value,
                                     S.deadline, S.sims_run, e->stream);
        }))
        return rc;
    e->last.sims = S.sims;  // (with a budget: replaced by the games' largest count when it is asked for)
    return 0;
}

// k_search_par: the whole leaf-parallel search in one launch.
static int search_par(oaz_engine* e, const Search& S) {
    e->times.parts = 1;
    const ParBufs b{e->par_path,   e->par_depth, e->par_leaf,  e->par_state,
                    e->par_policy, e->par_value, e->par_stats, (uint32_t)e->cfg.leaf_batch};
    if (int rc = timed(e, K_BACKUP_SELECT, S.t.G, [&] {
            return launch_search_par(S.t, S.roots, S.prm, (int)S.sims, S.net, b, S.deadline, S.sims_run, e->stream);
        }))
        return rc;
    e->par_G = S.t.G;
    e->last.sims = S.sims;  // (with a budget: replaced by the roots' largest count when it is asked for)
    return 0;
}

// An engine with leaf_batch > 0 runs k_search_par or nothing: the searches it cannot take fail here, before
// anything is launched.
static int par_search_check(const oaz_engine* e, uint32_t G, const char* who) {
    if (e->cfg.leaf_batch == 0) return 0;
    if (e->cfg.train_noise)
        return oaz_set_err(OAZ_ERR_STATE, "%s: leaf_batch=%d does not run with root noise (train_noise = 1)", who,
                           e->cfg.leaf_batch);
    if (G > (uint32_t)e->cus)
        return oaz_set_err(OAZ_ERR_STATE, "%s: leaf_batch=%d searches at most %d roots (one workgroup per CU), got %u", who,
                           e->cfg.leaf_batch, e->cus, G);
    return 0;
}

// k_search_grp: chunk c's simulations in one launch (the one part: every game, on the engine stream), each
// workgroup walking, evaluating and backing up its 16 games without a grid-wide step.
static int grp_chunk(oaz_engine* e, const Search& S, const NoiseRing& ring, uint32_t c) {
    const uint32_t s0 = c * ring.chunk, s1 = std::min(s0 + ring.chunk, S.sims);
    if (int rc = timed(e, K_BACKUP_SELECT, S.t.G * (s1 - s0), [&] {
            return launch_search_grp(S.t, S.roots, S.active, S.prm, (int)s0, (int)s1, ring.at(s0, 0), S.net, e->policy,
                                     e->value, S.deadline, S.sims_run, e->stream);
        }))
        return rc;
    e->last.sims = s1;
    return 0;
}

// Simulation step s for every part, in lock step: select -> leaf compaction -> evaluate -> expand/backup,
// where simulation s - 1's expand/backup and simulation s's select run as one kernel (k_backup_select_seg; a
// game's next walk needs only its own backup; the last simulation's expand/backup is run_chunks'). Select
// marks the games whose playout uses its leaf evaluation (all but those ending on a won, terminal-flagged
// node, whose evaluation the reference discards: mcts_arena.rs:156-176) and the compaction kernel packs their
// leaves per 4096-game bucket, so the network evaluates only those.
// Q7 on this loop (larger batches), which advances all games together: the host clock is read between
// simulation steps and the search stops (*spent) after the first step that ends at or past the budget, so
// every game has run the same number of playouts (>= 1); pi / the move come from the visits that ran. This
// waits for every part's stream before each simulation step, so a budgeted search gives up the parts' overlap
// (and the root-noise producer runs ahead at most to the step being waited on) and is not the one-launch
// search: its throughput is not comparable with an unbudgeted run's (the reference's own cutoff is a clock
// read per playout, mcts_arena.rs:78). Parity runs and the benches leave it off.
static int sim_step(oaz_engine* e, const Search& S, const Parts& P, const NoiseRing& ring, uint32_t s, bool* spent) {
    if (e->cfg.search_time_ns > 0 && s > 0) {
        for (int h = 0; h < P.n; ++h) HIP_TRY(hipStreamSynchronize(P.part[h].st));
        if ((*spent = now_ns() - e->t_search0 >= (double)e->cfg.search_time_ns)) return 0;
    }
    e->last.sims = s + 1;
    // sampled steps sit mid-chunk: a chunk's first select also waits for its noise
    e->timing_skip = e->timing_every > 1 && s % (uint32_t)e->timing_every != (uint32_t)e->timing_every / 2;
    for (int h = 0; h < P.n; ++h) {
        const Parts::Part& p = P.part[h];
        const noise_t* nz = ring.at(s, p.g0);
        if (s == 0) {
            if (int rc = timed(e, K_SELECT, p.t.G, [&] {
                    return launch_select(p.t, p.roots, p.active, nz, S.prm, p.st);
                }, p.st))
                return rc;
        } else if (int rc = timed(e, K_BACKUP_SELECT, p.t.G, [&] {
                       return launch_backup_select(p.t, p.roots, p.active, p.pol, p.val, nz, S.prm, p.st);
                   }, p.st)) {
            return rc;
        }
        if (!p.t.need) {
            if (int rc = evaluate(e, p.t.leaf_state, p.t.G, p.pol, p.val, p.st)) return rc;
            continue;
        }
        // row loads clamped to the part's own rows (the next part's compaction writes its rows on another stream)
        const TileMap tm{p.t.bcnt, buckets_of(p.t.G), (int32_t)p.t.G};
        if (int rc = timed(e, K_COMPACT, p.t.G, [&] { return launch_eval_compact(p.t, p.st); }, p.st)) return rc;
        if (int rc = evaluate(e, p.t.cstate, p.t.G, p.pol, p.val, p.st, &tm)) return rc;
    }
    return 0;
}

// The search chunk by chunk of the root-noise ring (one chunk = e->noise_chunk simulations, with or without
// noise): per chunk one k_search_grp launch (grp), or its simulation steps over the game parts. Ends with the
// last simulation's expand/backup per part and the parts' streams joined into the engine stream.
static int run_chunks(oaz_engine* e, const Search& S, bool grp) {
    const Parts P(e, S, grp ? 1 : game_parts(e, S.t.G));
    const NoiseRing ring{e, S, P, e->noise_chunk};
    const uint32_t nchunks = (S.sims + ring.chunk - 1) / ring.chunk;
    e->times.parts = (uint64_t)P.n;
    if (int rc = ring.produce(0)) return rc;
    if (int rc = P.fork()) return rc;
    bool spent = false;
    for (uint32_t c = 0; c < nchunks && !spent; ++c) {
        if (int rc = ring.produce(c + 1)) return rc;
        if (int rc = ring.wait(c)) return rc;
        if (grp) {
            if (int rc = grp_chunk(e, S, ring, c)) return rc;
        } else {
            for (uint32_t s = c * ring.chunk, s1 = std::min(s + ring.chunk, S.sims); s < s1 && !spent; ++s)
                if (int rc = sim_step(e, S, P, ring, s, &spent)) return rc;
        }
        if (int rc = ring.release(c)) return rc;
    }
    e->timing_skip = false;
    for (int h = 0; h < P.n; ++h) {
        const Parts::Part& p = P.part[h];
        if (int rc = timed(e, K_EXPAND, p.t.G, [&] {
                return launch_expand_backup(p.t, p.roots, p.active, p.pol, p.val, p.st);
            }, p.st))
            return rc;
    }
    return P.join();
}

// The two budget phases of a capped self-play ply (playout cap randomization): the playouts
// of a fast ply and the two masks launch_playout_cap_masks made of the slots' `active` bytes for this ply.
struct PlyCap {
    uint32_t n;            // fast_sims, 1 <= n < S.sims
    const uint8_t* fast;   // [G] active and a fast ply: these games stop after simulation n - 1
    const uint8_t* fullm;  // [G] active and a full ply: these go on to S.sims
};

// A capped ply on the per-step loop, leaf compaction on: run_chunks' per-step branch with the mask changing once.
//   steps 0 .. n-1       every active game (S.active), as without a cap;
//   expand/backup        simulation n - 1's, for the games that stop (fast), on each part's own stream and queued
//                        before step n: it reads the rows step n - 1's compaction left in `slot`, which step n's
//                        compaction rewrites;
//   steps n .. sims-1    the full games (fullm): to every kernel a fast game is now an idle slot, so its `need` byte
//                        is 0 and its leaf is in no network tile. Step n's fused backup/select backs simulation
//                        n - 1 up for exactly the games it then walks;
//   expand/backup        the last simulation's, for the full games.
// The host does not know whether any game's ply is a full one, so the second phase is always launched; with no full
// game its tree kernels find idle slots only and the network's workgroups exit on empty buckets. The root-noise
// chunks that begin at or after simulation n are drawn for the full games only.
static int run_capped(oaz_engine* e, const Search& S0, const PlyCap& pc) {
    Search S = S0;  // (the ring's producer reads S.active when a chunk is launched)
    Parts P(e, S, game_parts(e, S.t.G));
    const NoiseRing ring{e, S, P, e->noise_chunk};
    const uint32_t nchunks = (S.sims + ring.chunk - 1) / ring.chunk;
    e->times.parts = (uint64_t)P.n;
    const auto backup = [&](const uint8_t* mask) {
        e->timing_skip = false;
        for (int h = 0; h < P.n; ++h) {
            const Parts::Part& p = P.part[h];
            if (int rc = timed(e, K_EXPAND, p.t.G, [&] {
                    return launch_expand_backup(p.t, p.roots, mask + p.g0, p.pol, p.val, p.st);
                }, p.st))
                return rc;
        }
        return 0;
    };
    if (int rc = ring.produce(0)) return rc;
    if (int rc = P.fork()) return rc;
    bool spent = false;  // (never set: a capped ply has no search-time budget)
    for (uint32_t c = 0; c < nchunks; ++c) {
        if ((c + 1) * ring.chunk >= pc.n) S.active = pc.fullm;
        if (int rc = ring.produce(c + 1)) return rc;
        if (int rc = ring.wait(c)) return rc;
        for (uint32_t s = c * ring.chunk, s1 = std::min(s + ring.chunk, S.sims); s < s1; ++s) {
            if (s == pc.n) {
                if (int rc = backup(pc.fast)) return rc;
                for (int h = 0; h < P.n; ++h) P.part[h].active = pc.fullm + P.part[h].g0;
            }
            if (int rc = sim_step(e, S, P, ring, s, &spent)) return rc;
        }
        if (int rc = ring.release(c)) return rc;
    }
    if (int rc = backup(pc.fullm)) return rc;
    return P.join();
}

// The simulations of one move on the path that fits (search_path). On an error the game parts' streams are
// joined into the engine stream anyway (all of them, whatever the number of parts was: the drivers' early
// returns skip the join), so oaz_sync and buffer reuse after an error wait for them.
// pc (a capped self-play ply): run_capped, whatever cfg.compact and cfg.step_kernels say; the forced path is only
// there for the work it saves.
static int run_sims(oaz_engine* e, const TreeView& t, const oaz_state* roots, const uint8_t* active,
                    const uint64_t* gids, const uint32_t* plies, bool kept_trees = false, const PlyCap* pc = nullptr) {
    const bool budget = e->cfg.search_time_ns > 0, noise = e->cfg.train_noise && e->noise;
    const SearchPath path = pc ? PATH_STEPS : search_path(e, t.G, noise, kept_trees);
    const NNView w = nn_view(e, nullptr);
    Search S{t, roots, active, gids, plies, search_params(e), (uint32_t)e->cfg.sims, noise,
             e->cfg.evaluator == OAZ_EVAL_HASH ? nullptr : &w, budget ? e->deadline.get() : nullptr,
             budget ? e->sims_run.get() : nullptr};
    if (!pc && !compact_leaves(e, t.G)) {  // (always so on the one-launch paths) rows = game ids
        S.t.need = nullptr;
        S.t.slot = nullptr;
    }
    e->last = LastSearch{t.G};
    int rc = path == PATH_STEPS ? 0 : arm_device_budget(e, t.G);
    if (!rc)
        rc = pc                 ? run_capped(e, S, *pc)
             : path == PATH_PAR ? search_par(e, S)
             : path == PATH_LAT ? search_lat(e, S)
                                : run_chunks(e, S, path == PATH_GRP);
    if (rc) {
        const std::string msg = g_err;
        for (int h = 1; h < kMaxParts; ++h)
            if (hipEventRecord(e->ev_part[h], e->stream3[h - 1]) == hipSuccess)
                (void)hipStreamWaitEvent(e->stream, e->ev_part[h], 0);
        e->timing_skip = false;
        g_err = msg;
    }
    return rc;
}

static int reduce_stats(oaz_engine* e, uint32_t G, uint64_t out[GS_COUNT]) {
    HIP_TRY(launch_stats_reduce(e->stats, G, e->stats_sum, e->stream));
    HIP_TRY(hipMemcpyAsync(out, e->stats_sum, GS_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

static void fill_search_stats(const uint64_t* s, oaz_search_stats* o) {
    o->sims = s[GS_SIMS];
    o->expansions = s[GS_EXPANSIONS];
    o->children = s[GS_CHILDREN];
    o->terminal_leaves = s[GS_TERMINAL];
    o->depth_sum = s[GS_DEPTH];
    o->stuck_leaves = s[GS_STUCK];
    o->max_nodes = s[GS_MAXNODES];
    o->nn_evals = s[GS_EVALS];
}

// The search of G roots, enqueued on the engine stream (on the engine's device): `roots` (host) are uploaded
// to s_roots first, or with roots == null the G positions already in s_roots are searched (the arena's
// device-resident fight, oaz_arena.hip). The moves are left in s_move and pi in s_pi. Without a search_time
// budget nothing here waits for the device.
// keep_trees (oaz_search_resume): no tree reset; the playouts go on with the first G trees as they are. Any
// search ends what tree reuse may go on from (`searched` = 0); oaz_search and oaz_search_resume, the two searches
// oaz_search_advance follows, set it again (searched_trees), the arena's resident search does not.
static int search_core(oaz_engine* e, const oaz_state* roots, int G, bool keep_trees = false) {
    if (int rc = par_search_check(e, (uint32_t)G, "search")) return rc;
    e->ply_trees = false;
    e->searched = 0;
    if (int rc = begin_budget(e)) return rc;
    const TreeView t = tree_view(e, (uint32_t)G);
    if (roots) HIP_TRY(hipMemcpyAsync(e->s_roots, roots, (size_t)G * sizeof(oaz_state), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(e->stats, 0, (size_t)G * GS_COUNT * sizeof(uint64_t), e->stream));
    // every root's "ply" (the root-noise key) is the number of this engine's earlier searches
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)e->s_ply.get(), (int)e->search_calls, (size_t)G, e->stream));
    e->search_calls++;
    if (!keep_trees) HIP_TRY(launch_tree_reset(t, e->stream));
    if (int rc = run_sims(e, t, e->s_roots, nullptr, nullptr, e->s_ply, keep_trees)) return rc;
    return timed(e, K_FINALIZE, (uint32_t)G,
                 [&] { return launch_search_finalize(t, e->s_roots, e->s_move, e->s_pi, e->stream); });
}

// Engine internals used by the arena (oaz_arena.hip, declared in oaz_host.h).
int oaz_engine_arena_view(oaz_engine* e, oaz_arena_engine_view* out) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "arena: null engine");
    out->device = e->device;
    out->games = e->G;
    out->roots = e->s_roots;
    out->moves = e->s_move;
    out->stream = e->stream;
    return 0;
}
int oaz_engine_search_resident(oaz_engine* e, int G) {
    if (!e || G < 0 || (uint32_t)G > e->G) return oaz_set_err(OAZ_ERR_CAPACITY, "arena: %d roots > the engine's games", G);
    return G == 0 ? 0 : search_core(e, nullptr, G);
}

// After search_core in oaz_search / oaz_search_resume: the first G trees are what oaz_search_advance may re-root,
// and hold at most `visits` root visits.
static void searched_trees(oaz_engine* e, int G, int64_t visits) {
    e->searched = (uint32_t)G;
    e->tree_visits = visits;
}

// What oaz_search and oaz_search_resume hand back after search_core: the optional extra root evaluation, the
// moves, pi and resident roots to the host, then the statistics. Waits for the engine stream.
static int search_results(oaz_engine* e, int G, oaz_move* out_move, float* out_pi, float* out_root_value,
                          oaz_search_stats* stats, oaz_state* out_roots) {
    if (out_roots) HIP_TRY(hipMemcpyAsync(out_roots, e->s_roots, (size_t)G * sizeof(oaz_state), hipMemcpyDeviceToHost, e->stream));
    if (out_root_value) {  // extra root evaluation (alphazero_mcts/mod.rs:137-141)
        if (int rc = evaluate(e, e->s_roots, (uint32_t)G, e->s_rootp, e->s_rootv)) return rc;
        HIP_TRY(hipMemcpyAsync(out_root_value, e->s_rootv, (size_t)G * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (out_move) HIP_TRY(hipMemcpyAsync(out_move, e->s_move, (size_t)G * sizeof(oaz_move), hipMemcpyDeviceToHost, e->stream));
    if (out_pi) HIP_TRY(hipMemcpyAsync(out_pi, e->s_pi, (size_t)G * 50 * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) {
        uint64_t s[GS_COUNT];
        if (int rc = reduce_stats(e, (uint32_t)G, s)) return rc;
        memset(stats, 0, sizeof(*stats));
        fill_search_stats(s, stats);
    }
    return 0;
}

extern "C" int oaz_search(oaz_engine* e, const oaz_state* roots, int G, oaz_move* out_move, float* out_pi,
                          float* out_root_value, oaz_search_stats* stats) {
    if (!e || !roots || G < 0) return oaz_set_err(OAZ_ERR_ARG, "search: bad arguments");
    if ((uint32_t)G > e->G) return oaz_set_err(OAZ_ERR_CAPACITY, "search: G=%d > games=%u", G, e->G);
    if (G == 0) return 0;
    for (int i = 0; i < G; ++i)
        if (roots[i].to_move > 1) return oaz_set_err(OAZ_ERR_ARG, "search: root %d has to_move=%d", i, roots[i].to_move);
    OAZ_ON_DEVICE(e->device);
    if (int rc = search_core(e, roots, G)) {
        (void)hipStreamSynchronize(e->stream);  // the roots upload reads the caller's buffer
        return rc;
    }
    searched_trees(e, G, e->cfg.sims);
    return search_results(e, G, out_move, out_pi, out_root_value, stats, nullptr);
}

// Tree reuse: oaz_search on the resident roots, going on with the trees as oaz_search_advance left them.
extern "C" int oaz_search_resume(oaz_engine* e, int G, oaz_move* out_move, float* out_pi, float* out_root_value,
                                 oaz_search_stats* stats, oaz_state* out_roots) {
    if (!e || G < 0) return oaz_set_err(OAZ_ERR_ARG, "search_resume: bad arguments");
    if (e->cfg.reuse_visits <= 0) return oaz_set_err(OAZ_ERR_STATE, "search_resume: the engine was made with reuse_visits = 0");
    if ((uint32_t)G > e->searched)
        return oaz_set_err(OAZ_ERR_STATE, "search_resume: G=%d, but the trees of %u games are the last search's", G, e->searched);
    if (e->tree_visits + e->cfg.sims > e->cfg.reuse_visits)
        return oaz_set_err(OAZ_ERR_STATE, "search_resume: %lld root visits + %d playouts exceed reuse_visits=%d",
                           (long long)e->tree_visits, e->cfg.sims, e->cfg.reuse_visits);
    if (G == 0) return 0;
    OAZ_ON_DEVICE(e->device);
    const int64_t visits = e->tree_visits + e->cfg.sims;
    if (int rc = search_core(e, nullptr, G, true)) return rc;
    searched_trees(e, G, visits);
    return search_results(e, G, out_move, out_pi, out_root_value, stats, out_roots);
}

// Engine internals used by tree reuse (oaz_tree_reuse.hip, declared in oaz_host.h).
int oaz_engine_reuse_view(oaz_engine* e, oaz_reuse_engine_view* out) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "tree reuse: null engine");
    *out = {e->device, e->searched, e->cap, e->cfg.reuse_visits, e->sims_cap, e->nodes, e->n_nodes, e->s_roots,
            e->adv_moves, e->adv_codes, e->adv_kept, e->reuse_cnt, e->stream, e->cfg.seed};
    return 0;
}
int oaz_engine_reuse_advanced(oaz_engine* e, int G, int32_t most) {
    e->searched = (uint32_t)G;
    e->tree_visits = most;
    return 0;
}

extern "C" int oaz_tree_dump(oaz_engine* e, int game, oaz_node* out, int cap, int* n_nodes) {
    if (!e || game < 0 || (uint32_t)game >= e->G) return oaz_set_err(OAZ_ERR_ARG, "tree_dump: bad game");
    OAZ_ON_DEVICE(e->device);
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, e->n_nodes + game, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_nodes) *n_nodes = (int)n;
    if (out && cap > 0) {
        const size_t m = n < (uint32_t)cap ? n : (uint32_t)cap;
        HIP_TRY(hipMemcpyAsync(out, e->nodes + (size_t)game * e->cap, m * sizeof(oaz_node), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return 0;
}

// ---- self-play ----------------------------------------------------------------------------------
// Self-play is not part of the leaf-parallel search: such an engine refuses it (no other algorithm runs instead).
static int par_no_selfplay(const oaz_engine* e, const char* who) {
    if (e->cfg.leaf_batch == 0) return 0;
    return oaz_set_err(OAZ_ERR_STATE, "%s: the engine was made with leaf_batch=%d, which searches only (no self-play)",
                       who, e->cfg.leaf_batch);
}

extern "C" int oaz_selfplay_reset(oaz_engine* e) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "selfplay_reset: null");
    if (int rc = par_no_selfplay(e, "selfplay_reset")) return rc;
    OAZ_ON_DEVICE(e->device);
    const TreeView t = tree_view(e, e->G);
    HIP_TRY(hipMemsetAsync(e->stats, 0, (size_t)e->G * GS_COUNT * sizeof(uint64_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->out_count, 0, sizeof(unsigned long long), e->stream));
    e->out_read = 0;
    if (e->reuse_cnt) HIP_TRY(hipMemsetAsync(e->reuse_cnt, 0, 4 * sizeof(uint64_t), e->stream));
    if (e->temp_cnt) HIP_TRY(hipMemsetAsync(e->temp_cnt, 0, 2 * sizeof(uint64_t), e->stream));
    if (e->pc_nrec) {
        HIP_TRY(hipMemsetAsync(e->pc_nrec, 0, (size_t)e->G * sizeof(uint32_t), e->stream));
        HIP_TRY(hipMemsetAsync(e->pc_cnt, 0, 2 * sizeof(unsigned long long), e->stream));
    }
    e->ply_trees = false;
    e->searched = 0;
    HIP_TRY(launch_selfplay_reset(t, slot_view(e), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->selfplay_ready = true;
    return 0;
}

extern "C" int oaz_selfplay_step(oaz_engine* e, int moves) {
    if (!e || moves < 0) return oaz_set_err(OAZ_ERR_ARG, "selfplay_step: bad arguments");
    if (int rc = par_no_selfplay(e, "selfplay_step")) return rc;
    const bool capped = e->pc_fast > 0;
    if (capped && e->pc_fast >= e->cfg.sims)
        return oaz_set_err(OAZ_ERR_STATE, "selfplay_step: the playout cap's fast_sims=%d is not below sims=%d", e->pc_fast,
                           e->cfg.sims);
    if (capped && e->cfg.search_time_ns > 0)
        return oaz_set_err(OAZ_ERR_STATE, "selfplay_step: a playout cap does not run with a search-time budget");
    if (!e->selfplay_ready)
        if (int rc = oaz_selfplay_reset(e)) return rc;
    OAZ_ON_DEVICE(e->device);
    const TreeView t = tree_view(e, e->G);
    const SlotView sv = slot_view(e);
    const uint32_t temp_plies = e->cfg.temperature_plies;  // 0: the launches of an engine without temperature
    const CapView cv = cap_view(e);  // (all null without a cap)
    const PlyCap pc{(uint32_t)e->pc_fast, cv.fast, cv.fullm};
    for (int m = 0; m < moves; ++m) {
        if (int rc = begin_budget(e)) return rc;
        const bool reuse = e->cfg.reuse_visits > 0;
        e->searched = 0;
        if (!reuse)
            HIP_TRY(launch_tree_reset(t, e->stream));  // a fresh tree per move (the last ply's stays dumpable)
        else  // tree reuse: the played move's subtree where the keep rule holds, a fresh root elsewhere
            HIP_TRY(launch_selfplay_rebase(t, sv, e->ply_trees, e->sims_cap, e->cfg.reuse_visits, temp_plies, e->reuse_cnt,
                                           e->stream));
        e->ply_trees = false;
        if (capped) HIP_TRY(launch_playout_cap_masks(sv, cv, e->stream));  // this ply's full flags and phase masks
        if (int rc = run_sims(e, t, e->root, e->active, e->game_id, e->ply, reuse, capped ? &pc : nullptr)) return rc;
        if (int rc = timed(e, K_FINALIZE, e->G, [&] {
                return capped       ? launch_selfplay_move_cap(t, sv, cv, temp_plies, e->temp_cnt, e->stream)
                       : temp_plies ? launch_selfplay_move_temp(t, sv, temp_plies, e->temp_cnt, e->stream)
                                    : launch_selfplay_move(t, sv, e->stream);
            }))
            return rc;
        e->ply_trees = true;
    }
    return 0;
}

// How many samples are ready: of the *avail records in the buffer after the engine stream's work so far (the
// device's counter runs past out_cap when records were dropped), those not handed out yet.
static int samples_ready(oaz_engine* e, size_t* ready, unsigned long long* avail) {
    unsigned long long cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, e->out_count, sizeof(cnt), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *avail = cnt < e->out_cap ? cnt : e->out_cap;
    *ready = *avail > e->out_read ? (size_t)(*avail - e->out_read) : 0;
    return 0;
}

// Advances the read cursor by n of the `avail` samples (samples_ready) and rewinds the buffer once it is drained.
static int samples_advance(oaz_engine* e, size_t n, unsigned long long avail) {
    e->out_read += n;
    if (e->out_read == avail) {
        HIP_TRY(hipMemsetAsync(e->out_count, 0, sizeof(unsigned long long), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->out_read = 0;
    }
    return 0;
}

extern "C" int oaz_selfplay_stats_get(oaz_engine* e, oaz_selfplay_stats* o) {
    if (!e || !o) return oaz_set_err(OAZ_ERR_ARG, "selfplay_stats: null");
    OAZ_ON_DEVICE(e->device);
    uint64_t s[GS_COUNT];
    if (int rc = reduce_stats(e, e->G, s)) return rc;
    size_t ready = 0;
    unsigned long long avail = 0;
    if (int rc = samples_ready(e, &ready, &avail)) return rc;
    memset(o, 0, sizeof(*o));
    o->moves = s[GS_MOVES];
    o->games_finished = s[GS_FINISHED];
    o->games_cut = s[GS_CUT];
    o->red_wins = s[GS_RED];
    o->blue_wins = s[GS_BLUE];
    o->passes = s[GS_PASSES];
    o->samples_dropped = s[GS_DROPPED];
    o->samples_ready = ready;
    fill_search_stats(s, &o->search);
    return 0;
}

extern "C" int oaz_selfplay_temperature_stats(oaz_engine* e, uint64_t out[2]) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "selfplay_temperature_stats: null");
    out[0] = out[1] = 0;
    if (!e->temp_cnt) return 0;
    OAZ_ON_DEVICE(e->device);
    HIP_TRY(hipMemcpyAsync(out, e->temp_cnt, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// ---- playout cap randomization ---------------------------------------------------------
extern "C" int oaz_playout_cap_full(uint64_t seed, uint64_t game_id, uint32_t ply, uint32_t full_per_65536) {
    if (full_per_65536 > 65536u)
        return oaz_set_err(OAZ_ERR_ARG, "playout_cap_full: full_per_65536=%u > 65536", full_per_65536);
    return playout_cap_full(seed, game_id, ply, full_per_65536) ? 1 : 0;
}

// An engine setting, as oaz_set_search_time is (oaz_config keeps its size). The combinations the two-phase ply does
// not run are refused here or at the step; nothing else runs in its place.
extern "C" int oaz_selfplay_set_playout_cap(oaz_engine* e, int fast_sims, int full_per_65536) {
    if (!e) return oaz_set_err(OAZ_ERR_ARG, "set_playout_cap: null");
    if (fast_sims < 0 || full_per_65536 < 0 || full_per_65536 > 65536)
        return oaz_set_err(OAZ_ERR_ARG, "set_playout_cap: fast_sims=%d, full_per_65536=%d (>= 0, 0 .. 65536)", fast_sims,
                           full_per_65536);
    if (fast_sims > 0) {
        if (e->cfg.reuse_visits > 0)
            return oaz_set_err(OAZ_ERR_STATE, "set_playout_cap: the engine was made with reuse_visits=%d (tree reuse)",
                               e->cfg.reuse_visits);
        if (e->cfg.leaf_batch > 0)
            return oaz_set_err(OAZ_ERR_STATE, "set_playout_cap: the engine was made with leaf_batch=%d (no self-play)",
                               e->cfg.leaf_batch);
        if (e->cfg.search_time_ns > 0)
            return oaz_set_err(OAZ_ERR_STATE, "set_playout_cap: the engine has a search-time budget");
        if (!launch_playout_cap_masks || !launch_selfplay_move_cap)
            return oaz_set_err(OAZ_ERR_STATE, "set_playout_cap: built without the playout cap kernels");
        if (!e->pc_flags) {  // its buffers come with the first cap, not at creation
            OAZ_ON_DEVICE(e->device);
            if (e->pc_flags.alloc(3 * (size_t)e->G) || e->pc_nrec.alloc(e->G) || e->pc_cnt.alloc(2)) return OAZ_ERR_HIP;
        }
    }
    if (fast_sims == e->pc_fast && (uint32_t)full_per_65536 == e->pc_share) return 0;
    e->pc_fast = fast_sims;
    e->pc_share = (uint32_t)full_per_65536;
    e->selfplay_ready = false;  // the running games end: the next oaz_selfplay_step starts from a reset
    if (e->pc_cnt) {            // (which also clears these; until then the counters read 0)
        OAZ_ON_DEVICE(e->device);
        HIP_TRY(hipMemsetAsync(e->pc_cnt, 0, 2 * sizeof(unsigned long long), e->stream));
    }
    return 0;
}

extern "C" int oaz_selfplay_playout_cap_stats(oaz_engine* e, uint64_t out[2]) {
    if (!e || !out) return oaz_set_err(OAZ_ERR_ARG, "selfplay_playout_cap_stats: null");
    out[0] = out[1] = 0;
    if (e->pc_fast == 0) return 0;
    OAZ_ON_DEVICE(e->device);
    HIP_TRY(hipMemcpyAsync(out, e->pc_cnt, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

static int samples_copy(oaz_engine* e, void* dst, size_t cap, size_t* n_out, hipMemcpyKind kind) {
    OAZ_ON_DEVICE(e->device);
    size_t ready = 0;
    unsigned long long avail = 0;
    if (int rc = samples_ready(e, &ready, &avail)) return rc;
    const size_t n = ready < cap ? ready : cap;
    if (n) HIP_TRY(hipMemcpyAsync(dst, e->out + e->out_read, n * sizeof(oaz_sample), kind, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rc = samples_advance(e, n, avail)) return rc;
    if (n_out) *n_out = n;
    return 0;
}

// Internal (oaz_host.h), for oaz_allgather_samples: the engine's buffered samples as one contiguous
// device range [*dev, *dev + *n), after the engine's work so far is complete.
int oaz_engine_samples_peek(oaz_engine* e, const oaz_sample** dev, size_t* n, int* device) {
    OAZ_ON_DEVICE(e->device);
    HIP_TRY(hipStreamSynchronize(e->stream2));
    unsigned long long avail = 0;
    if (int rc = samples_ready(e, n, &avail)) return rc;
    *dev = e->out + e->out_read;
    *device = e->device;
    return 0;
}

// Drops the first n peeked samples (the caller's copies of them are complete).
int oaz_engine_samples_consume(oaz_engine* e, size_t n) {
    OAZ_ON_DEVICE(e->device);
    size_t ready = 0;
    unsigned long long avail = 0;
    if (int rc = samples_ready(e, &ready, &avail)) return rc;
    return samples_advance(e, n, avail);
}

extern "C" int oaz_samples_fetch(oaz_engine* e, oaz_sample* out, size_t cap, size_t* n_out) {
    if (!e || (!out && cap)) return oaz_set_err(OAZ_ERR_ARG, "samples_fetch: bad arguments");
    return samples_copy(e, out, cap, n_out, hipMemcpyDeviceToHost);
}

extern "C" int oaz_samples_export_device(oaz_engine* e, void* dev_dst, size_t cap_bytes, size_t* n_out) {
    if (!e || (!dev_dst && cap_bytes)) return oaz_set_err(OAZ_ERR_ARG, "samples_export: bad arguments");
    return samples_copy(e, dev_dst, cap_bytes / sizeof(oaz_sample), n_out, hipMemcpyDeviceToDevice);
}

// Games of the first `quota` global ids that this rank plays: rank r owns the ids
// seq * world * G + r * G + g (g < G, seq >= 0; SlotView, k_selfplay_move).
static uint64_t rank_share(const oaz_engine* e, uint64_t quota) {
    const uint64_t G = e->G, W = (uint64_t)(e->cfg.world > 0 ? e->cfg.world : 1), r = (uint64_t)e->cfg.rank;
    const uint64_t full = quota / (W * G), rem = quota % (W * G);
    const uint64_t lo = r * G;
    return full * G + (rem > lo ? (rem - lo < G ? rem - lo : G) : 0);
}

extern "C" int oaz_selfplay_run(oaz_engine* e, int n_games, oaz_sample* out, size_t cap, size_t* n_out,
                                oaz_selfplay_stats* stats) {
    if (!e || n_games < 0) return oaz_set_err(OAZ_ERR_ARG, "selfplay_run: bad arguments");
    if (int rc = par_no_selfplay(e, "selfplay_run")) return rc;
    e->quota = (uint64_t)n_games;  // slots stop dealing at global game index >= n_games
    const uint64_t mine = rank_share(e, e->quota);  // this rank's share of the n_games (global) games
    int rc = oaz_selfplay_reset(e);
    if (rc) {
        e->quota = 0;
        return rc;
    }
    size_t got = 0;
    for (;;) {
        oaz_selfplay_stats st;
        if ((rc = oaz_selfplay_stats_get(e, &st))) break;
        if (st.games_finished >= mine) {
            if (stats) *stats = st;
            break;
        }
        if ((rc = oaz_selfplay_step(e, 8))) break;
        size_t n = 0;
        if (out && got < cap) {
            if ((rc = oaz_samples_fetch(e, out + got, cap - got, &n))) break;
            got += n;
        }
    }
    if (!rc && out && got < cap) {
        size_t n = 0;
        rc = oaz_samples_fetch(e, out + got, cap - got, &n);
        got += n;
    }
    e->quota = 0;
    e->selfplay_ready = false;
    if (n_out) *n_out = got;
    return rc;
}
