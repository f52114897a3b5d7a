// oaz_arena.hip — the arena: a fight (alphazero-training/src/evaluator.rs:355-399) whose game states stay on the
// GPU, the Random agent (onitama-game/src/ai/random.rs) as a kernel, and the host-side Elo / FightStatistics fold.
//
// Per ply:  k_arena_route  ->  each side's batched search  ->  k_arena_apply per side.
//   * every game slot has its own fields (state, game id, ply count, ply budget, progress, active flag): the
//     kernels take what they need from the slot and never assume that the slots are at the same ply;
//   * k_arena_route compacts the active games, in ascending slot order, into the root buffer of the side that
//     moves in them (an AlphaZero side's is its engine's search-root buffer) with the slots' indices next to
//     them; the two counts (8 bytes, pinned memory) are all the host reads per ply, and both zero ends the fight;
//   * an AlphaZero side searches the roots where they are (oaz_engine_search_resident), a Random side runs
//     k_arena_random, both asynchronously on the side's stream, so the two sides of a ply overlap; pure-MCTS
//     and alpha-beta sides go through their host-pointer entry points with pinned staging buffers;
//   * k_arena_apply runs on the side's stream right after its search (the sides' games are disjoint), and the
//     next route waits for both sides' events;
//   * a fight on fewer slots than games (oaz_arena_fight_slots) runs k_arena_refill before every route: a slot
//     that finished stores its result under its game index and is dealt the fight's next game.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/onitama_az.h"
#include "oaz_device.h"
#include "oaz_host.h"

using namespace oaz;

static_assert(sizeof(oaz_arena_agent) == 88 && sizeof(oaz_arena_config) == 40 && sizeof(oaz_fight_stats) == 96 &&
                  sizeof(oaz_arena_slots_stats) == 40,
              "arena struct layout");

namespace oaz {
namespace arena {

__constant__ AttackTable c_attack = make_attack_table();

// The game slots of one fight.
struct Slots {
    oaz_state* state;   // [n] current position
    uint64_t* game;     // [n] game index of the fight: the agent plays Red when it is even; keys deal and Random draws
    int32_t* plies;     // [n] moves made = the ply the slot's next move is
    int32_t* budget;    // [n] max_plies, one less after every ply (evaluator.rs:376-389)
    uint32_t* passes;   // [n] passes among the moves
    uint8_t* progress;  // [n] last MoveResult
    uint8_t* active;    // [n] 1 = playing
    uint32_t n;
};

// One side's compacted roots of a ply.
struct SideBuf {
    oaz_state* roots;  // [cap]
    uint32_t* idx;     // [cap] slot of root i
    uint32_t cap;
};

__device__ __forceinline__ oaz_state load_state(const oaz_state* p) {
    oaz_state s;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    uint32_t* d = reinterpret_cast<uint32_t*>(&s);
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = q[i];
    return s;
}
__device__ __forceinline__ void store_state(oaz_state* p, const oaz_state& s) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(&s);
#pragma unroll
    for (int i = 0; i < 6; ++i) q[i] = d[i];
}

// 0: the agent moves in the slot, 1: the opponent, 2: nobody (finished)
__device__ __forceinline__ int slot_side(const Slots& v, uint32_t g) {
    if (!v.active[g]) return 2;
    const bool red_to_move = (v.state[g].to_move & 1) == 0, agent_red = (v.game[g] & 1) == 0;
    return red_to_move == agent_red ? 0 : 1;
}

// Ordered compaction in one workgroup (the shape of k_samples_scan): each thread counts a run of consecutive
// slots per side, the workgroup scans the runs in LDS (both sides' counts in one 64-bit word), and every
// thread writes its run's roots and slot indices from its offsets on. Writes are bounded by the buffers'
// capacities; the counts are the true ones, so the host sees an overflow.
constexpr int kRouteThreads = 1024;
__global__ void __launch_bounds__(kRouteThreads) k_arena_route(Slots v, SideBuf a, SideBuf b, uint32_t* counts) {
    const uint32_t per = (v.n + kRouteThreads - 1) / kRouteThreads;
    const uint32_t g0 = threadIdx.x * per < v.n ? threadIdx.x * per : v.n, g1 = g0 + per < v.n ? g0 + per : v.n;
    uint64_t sum = 0;  // agent's count | opponent's count << 32
    for (uint32_t g = g0; g < g1; ++g) {
        const int sd = slot_side(v, g);
        sum += sd == 0 ? 1ull : sd == 1 ? (1ull << 32) : 0ull;
    }
    __shared__ uint64_t run[kRouteThreads];
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kRouteThreads; d <<= 1) {  // inclusive Hillis-Steele scan of the runs
        const uint64_t t = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0ull;
        __syncthreads();
        run[threadIdx.x] += t;
        __syncthreads();
    }
    const uint64_t excl = run[threadIdx.x] - sum;
    uint32_t pa = (uint32_t)excl, pb = (uint32_t)(excl >> 32);
    for (uint32_t g = g0; g < g1; ++g) {
        const int sd = slot_side(v, g);
        if (sd == 2) continue;
        const SideBuf& o = sd == 0 ? a : b;
        const uint32_t p = sd == 0 ? pa++ : pb++;
        if (p < o.cap) {
            store_state(&o.roots[p], load_state(&v.state[g]));
            o.idx[p] = g;
        }
    }
    if (threadIdx.x == kRouteThreads - 1) {
        counts[0] = (uint32_t)run[kRouteThreads - 1];
        counts[1] = (uint32_t)(run[kRouteThreads - 1] >> 32);
    }
}

// Random::generate_move for every root of a side: one lane per root, random_agent_move (oaz_device.h).
constexpr int kLaneBlock = 256;
__global__ void __launch_bounds__(kLaneBlock) k_arena_random(Slots v, SideBuf sd, uint32_t cnt, uint64_t seed,
                                                             oaz_move* moves) {
    const uint32_t i = blockIdx.x * kLaneBlock + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t g = sd.idx[i];
    if (g >= v.n) return;
    const oaz_state s = load_state(&sd.roots[i]);
    oaz_move m;
    random_agent_move(c_attack, seed, v.game[g], (uint32_t)v.plies[g], s, m);
    moves[i] = m;
}

// The move or pass of root i in the slot its index names, and the slot's end-of-ply bookkeeping: the game ends
// on a win, or when the budget was already negative (checked before it is decremented).
__global__ void __launch_bounds__(kLaneBlock) k_arena_apply(Slots v, SideBuf sd, uint32_t cnt, const oaz_move* moves) {
    const uint32_t i = blockIdx.x * kLaneBlock + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t g = sd.idx[i];
    if (g >= v.n) return;
    oaz_state s = load_state(&v.state[g]);
    const oaz_move m = moves[i];
    int res = OAZ_IN_PROGRESS;
    if (m.from >= 25 || m.to >= 25) {  // pass (state.rs:139-142): the card goes round, nothing moves
        state_rotate(s, m.slot & 3);
        v.passes[g] += 1;
    } else {
        res = make_move_regs(s, m.from, m.to, m.piece & 1, m.slot & 3, s.to_move & 1);
    }
    s.to_move ^= 1;
    store_state(&v.state[g], s);
    v.progress[g] = (uint8_t)res;
    v.plies[g] += 1;
    const int32_t left = v.budget[g];
    v.budget[g] = left - 1;
    if (is_win(res) || left < 0) v.active[g] = 0;
}

// The games of a fight played on fewer slots than games (oaz_arena_fight_slots): where a game starts, where
// its result goes when its slot has finished it, and the first game that no slot has been dealt yet.
struct Games {
    const oaz_state* start;  // [n] game k's start position
    uint8_t* progress;       // [n] last MoveResult
    int32_t* plies;          // [n] moves made
    uint32_t* passes;        // [n] passes among them
    uint32_t* next;          // [1] first game not dealt
    uint32_t n;
    int32_t max_plies;
};
constexpr uint64_t kNoGame = ~0ull;  // Slots::game of a slot that holds no game

// Between two plies: every slot that finished its game stores the result under the game's index and is dealt
// the fight's next game, in ascending slot order. One workgroup in k_arena_route's shape: each thread counts
// the finished slots of its run, the scan of the runs ranks them, and the slot at rank r takes game next + r
// while there is one; a slot that gets none is empty from then on (kNoGame) and never harvested again. Every
// thread reads `next` before the scan's first barrier and the last thread writes it after the scan's last one.
__global__ void __launch_bounds__(kRouteThreads) k_arena_refill(Slots v, Games gm) {
    const uint32_t per = (v.n + kRouteThreads - 1) / kRouteThreads;
    const uint32_t g0 = threadIdx.x * per < v.n ? threadIdx.x * per : v.n, g1 = g0 + per < v.n ? g0 + per : v.n;
    const uint32_t next = *gm.next;
    uint32_t sum = 0;
    for (uint32_t g = g0; g < g1; ++g) sum += !v.active[g] && v.game[g] != kNoGame;
    __shared__ uint32_t run[kRouteThreads];
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kRouteThreads; d <<= 1) {  // inclusive Hillis-Steele scan of the runs
        const uint32_t t = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0u;
        __syncthreads();
        run[threadIdx.x] += t;
        __syncthreads();
    }
    uint64_t deal = (uint64_t)next + (run[threadIdx.x] - sum);  // the game this thread's next finished slot takes
    for (uint32_t g = g0; g < g1; ++g) {
        if (v.active[g]) continue;
        const uint64_t k = v.game[g];
        if (k == kNoGame) continue;
        if (k < gm.n) {
            gm.progress[k] = v.progress[g];
            gm.plies[k] = v.plies[g];
            gm.passes[k] = v.passes[g];
        }
        const uint64_t nk = deal++;
        if (nk < gm.n) {
            store_state(&v.state[g], load_state(&gm.start[nk]));
            v.game[g] = nk;
            v.plies[g] = 0;
            v.budget[g] = gm.max_plies;
            v.passes[g] = 0;
            v.progress[g] = (uint8_t)OAZ_IN_PROGRESS;
            v.active[g] = 1;
        } else {
            v.game[g] = kNoGame;
        }
    }
    if (threadIdx.x == kRouteThreads - 1) {
        const uint64_t nn = (uint64_t)next + run[kRouteThreads - 1];
        *gm.next = nn < gm.n ? (uint32_t)nn : gm.n;
    }
}

}  // namespace arena
}  // namespace oaz

// ---- host helpers (no GPU) ------------------------------------------------------------------------------
extern "C" void oaz_arena_config_default(oaz_arena_config* c) {  // evaluator.rs:129-136
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->game_amnt = 20;
    c->max_plies = 150;
    c->seed = 20260101;
}

extern "C" void oaz_elo_change(double ra, double rb, int a_won, double* ra_out, double* rb_out) {
    constexpr double kElo = 32.0, cElo = 2.5e-3;  // elo_rating.rs:52,54
    const double ea = 1.0 / (1.0 + pow(10.0, cElo * (rb - ra)));
    const double eb = 1.0 / (1.0 + pow(10.0, cElo * (ra - rb)));
    const double sa = a_won ? 1.0 : 0.0, sb = 1.0 - sa;
    if (ra_out) *ra_out = ra + kElo * (sa - ea);
    if (rb_out) *rb_out = rb + kElo * (sb - eb);
}

extern "C" int oaz_fight_stats_fold(const uint8_t* results, int n, double rating_a, double rating_b,
                                    oaz_fight_stats* out, double* history) {
    if (!out || n < 0 || (n > 0 && !results)) return oaz_set_err(OAZ_ERR_ARG, "fight_stats_fold: bad arguments");
    memset(out, 0, sizeof(*out));
    out->rating_a = rating_a;
    out->rating_b = rating_b;
    for (int k = 0; k < n; ++k) {
        const int r = results[k], color = k & 1;  // the agent is Red in even games
        if (r > OAZ_IN_PROGRESS) return oaz_set_err(OAZ_ERR_ARG, "fight_stats_fold: result %d of game %d", r, k);
        const bool won = r == (color ? OAZ_BLUE_WIN : OAZ_RED_WIN), lost = r == (color ? OAZ_RED_WIN : OAZ_BLUE_WIN);
        double ra = out->rating_a, rb = out->rating_b;
        if (won || lost) oaz_elo_change(out->rating_a, out->rating_b, won, &ra, &rb);
        if (history) {
            history[4 * k + 0] = out->rating_a;
            history[4 * k + 1] = ra;
            history[4 * k + 2] = out->rating_b;
            history[4 * k + 3] = rb;
        }
        out->rating_a = ra;
        out->rating_b = rb;
        if (won) {
            out->wins++;
            out->color_wins[color]++;
        } else if (lost) {
            out->loses++;
            out->color_loses[color]++;
        } else {
            out->draws++;
            out->color_draws[color]++;
        }
    }
    if (n > 0) {  // update_winrate (evaluator.rs:101-109) after the last update; 0 / 0 is NaN as in Rust
        out->winrate = (double)out->wins / (double)n;
        for (int c = 0; c < 2; ++c) {
            const uint32_t m = out->color_wins[c] + out->color_loses[c] + out->color_draws[c];
            out->color_winrate[c] = m ? (double)out->color_wins[c] / (double)m : (double)NAN;
        }
    }
    return 0;
}

extern "C" int oaz_random_agent_move(uint64_t seed, uint64_t game, uint32_t ply, const oaz_state* s, oaz_move* out) {
    if (!s || !out) return oaz_set_err(OAZ_ERR_ARG, "random_agent_move: null argument");
    if (!oaz_root_ok(*s, /*squares=*/false))  // (to_move and cards only: the squares are not looked at here)
        return oaz_set_err(OAZ_ERR_ARG, "random_agent_move: not a valid state");
    random_agent_move(kAttackHost, seed, game, ply, *s, *out);
    return 0;
}

static int check_arena_config(const oaz_arena_config* cfg) {
    if (!cfg) return oaz_set_err(OAZ_ERR_ARG, "arena: null config");
    if (cfg->game_amnt < 0) return oaz_set_err(OAZ_ERR_ARG, "arena: game_amnt %d", cfg->game_amnt);
    if (cfg->start) {  // (what the searches' own entry points ask of a root: squares 0..24, cards 0..15)
        for (int k = 0; k < cfg->game_amnt; ++k)
            if (!oaz_root_ok(cfg->start[k]))
                return oaz_set_err(OAZ_ERR_ARG, "arena: start position %d is not a valid state", k);
    } else if (cfg->fixed_deck) {
        uint32_t seen = 0;
        for (int i = 0; i < 5; ++i) {
            if (cfg->deck[i] >= OAZ_NUM_CARDS) return oaz_set_err(OAZ_ERR_ARG, "arena: deck card %d", cfg->deck[i]);
            if (seen & (1u << cfg->deck[i])) return oaz_set_err(OAZ_ERR_ARG, "arena: deck repeats card %d", cfg->deck[i]);
            seen |= 1u << cfg->deck[i];
        }
    }
    return 0;
}

// Game k's start position; need[s] = the largest batch side s answers (header, oaz_arena_capacity).
static void initial_states(const oaz_arena_config* cfg, std::vector<oaz_state>* out, int32_t need[2]) {
    const int n = cfg->game_amnt;
    if (out) out->resize((size_t)n);
    int32_t agent_first = 0;  // games whose first mover is the agent
    for (int k = 0; k < n; ++k) {
        oaz_state s;
        if (cfg->start) {
            s = cfg->start[k];
            s.pad[0] = s.pad[1] = 0;
        } else {
            uint8_t deck[5];
            if (cfg->fixed_deck) memcpy(deck, cfg->deck, 5);
            else deal_deck(cfg->seed, (uint64_t)k, deck);
            memset(&s, 0, sizeof(s));
            initial_state(deck, s);
        }
        agent_first += (s.to_move == OAZ_RED) == ((k & 1) == 0);
        if (out) (*out)[(size_t)k] = s;
    }
    need[0] = need[1] = agent_first > n - agent_first ? agent_first : n - agent_first;
}

extern "C" int oaz_arena_capacity(const oaz_arena_config* cfg, int32_t out[2]) {
    if (int rc = check_arena_config(cfg)) return rc;
    if (!out) return oaz_set_err(OAZ_ERR_ARG, "arena_capacity: null output");
    initial_states(cfg, nullptr, out);
    return 0;
}

extern "C" int oaz_arena_slots_capacity(const oaz_arena_config* cfg, int32_t slots, int32_t out[2]) {
    if (int rc = check_arena_config(cfg)) return rc;
    if (slots < 1) return oaz_set_err(OAZ_ERR_ARG, "arena: slots %d", slots);
    if (!out) return oaz_set_err(OAZ_ERR_ARG, "arena_slots_capacity: null output");
    if (slots >= cfg->game_amnt) initial_states(cfg, nullptr, out);  // nothing is refilled: the lock-step fight's
    else out[0] = out[1] = slots;  // slots at different plies can all be one side's turn
    return 0;
}

// ---- the fight --------------------------------------------------------------------------------------------
namespace {

struct Side {
    oaz_arena_agent ag;            // (a copy: device and game_id0 are the arena's)
    oaz_arena_engine_view ev{};    // ALPHAZERO
    arena::SideBuf buf{};          // roots: the engine's, or the fight's own
    oaz_move* moves = nullptr;     // the engine's s_move, or the fight's own
    oaz_state* staged = nullptr;   // the second side of a shared engine: routed here, copied to the engine's roots
    hipStream_t st = nullptr;      // the side's search and apply run here
    uint64_t calls = 0;            // searches so far (PURE_MCTS: game_id0 = calls << 20)
    bool blocking() const { return ag.kind == OAZ_AGENT_PURE_MCTS || ag.kind == OAZ_AGENT_ALPHABETA; }
};

// Owners in destruction order (oaz_host.h): streams first (destroyed last, after waiting), buffers, events.
struct Fight {
    Stream route;       // k_arena_route, uploads and read-backs
    Stream side_st[2];  // the sides without an engine
    DevBuf<char> dev;
    PinnedBuf<uint32_t> counts;
    PinnedBuf<oaz_state> h_roots[2];  // PURE_MCTS / ALPHABETA staging
    PinnedBuf<oaz_move> h_moves[2];
    std::vector<int32_t> h_score;     // (alpha-beta scores and pure-MCTS values nobody reads)
    Event done[2];                    // side s applied its moves of the ply
};

int check_side(const char* who, const oaz_arena_agent* a, const oaz_arena_config* cfg, int32_t need, Side* out) {
    if (!a) return oaz_set_err(OAZ_ERR_ARG, "arena: null %s", who);
    out->ag = *a;
    switch (a->kind) {
    case OAZ_AGENT_ALPHAZERO:
        if (!a->engine) return oaz_set_err(OAZ_ERR_ARG, "arena: the %s is OAZ_AGENT_ALPHAZERO without an engine", who);
        if (int rc = oaz_engine_arena_view(a->engine, &out->ev)) return rc;
        if (out->ev.device != cfg->device)
            return oaz_set_err(OAZ_ERR_ARG, "arena: the %s's engine is on device %d, the fight on %d", who, out->ev.device,
                               cfg->device);
        if ((int64_t)out->ev.games < (int64_t)need)
            return oaz_set_err(OAZ_ERR_CAPACITY, "arena: the %s's engine has %u games, the fight needs %d per ply", who,
                               out->ev.games, need);
        return 0;
    case OAZ_AGENT_RANDOM:
        return 0;
    case OAZ_AGENT_PURE_MCTS:
        if (a->mcts.max_playouts < 0 || a->mcts.min_node_visits < 0 || a->mcts.rollout_cap < 0)
            return oaz_set_err(OAZ_ERR_ARG, "arena: the %s's pure-MCTS config has a negative field", who);
        out->ag.mcts.device = cfg->device;
        return 0;
    case OAZ_AGENT_ALPHABETA:
        if (a->alphabeta.max_depth < 2 || a->alphabeta.max_depth > 6)
            return oaz_set_err(OAZ_ERR_ARG, "arena: the %s's alphabeta.max_depth %d outside 2..6", who, a->alphabeta.max_depth);
        out->ag.alphabeta.device = cfg->device;
        return 0;
    default:
        return oaz_set_err(OAZ_ERR_ARG, "arena: the %s has unknown kind %d", who, a->kind);
    }
}

hipError_t launch_apply(const arena::Slots& v, const Side& sd, uint32_t cnt) {
    hipLaunchKernelGGL(arena::k_arena_apply, dim3((cnt + arena::kLaneBlock - 1) / arena::kLaneBlock),
                       dim3(arena::kLaneBlock), 0, sd.st, v, sd.buf, cnt, sd.moves);
    return hipGetLastError();
}

// One side's moves of the ply for its cnt routed roots, then their application, on the side's stream.
int side_ply(Fight& f, const arena::Slots& v, Side& sd, int s, uint32_t cnt) {
    switch (sd.ag.kind) {
    case OAZ_AGENT_ALPHAZERO:
        if (sd.staged)
            HIP_TRY(hipMemcpyAsync(sd.ev.roots, sd.staged, (size_t)cnt * sizeof(oaz_state), hipMemcpyDeviceToDevice, sd.st));
        if (int rc = oaz_engine_search_resident(sd.ag.engine, (int)cnt)) return rc;
        break;
    case OAZ_AGENT_RANDOM:
        hipLaunchKernelGGL(arena::k_arena_random, dim3((cnt + arena::kLaneBlock - 1) / arena::kLaneBlock),
                           dim3(arena::kLaneBlock), 0, sd.st, v, sd.buf, cnt, sd.ag.seed, sd.moves);
        HIP_TRY(hipGetLastError());
        break;
    default: {  // PURE_MCTS / ALPHABETA: host-pointer entry points, roots down and moves up through pinned memory
        HIP_TRY(hipMemcpyAsync(f.h_roots[s].get(), sd.buf.roots, (size_t)cnt * sizeof(oaz_state), hipMemcpyDeviceToHost, sd.st));
        HIP_TRY(hipStreamSynchronize(sd.st));
        if (f.h_score.size() < cnt) f.h_score.resize(cnt);
        int rc;
        if (sd.ag.kind == OAZ_AGENT_PURE_MCTS) {
            sd.ag.mcts.game_id0 = sd.calls << 20;
            rc = oaz_pure_mcts_search(f.h_roots[s].get(), (int)cnt, &sd.ag.mcts, f.h_moves[s].get(),
                                      reinterpret_cast<float*>(f.h_score.data()), nullptr, nullptr, 0);
        } else {
            rc = oaz_alphabeta_search(f.h_roots[s].get(), (int)cnt, &sd.ag.alphabeta, f.h_moves[s].get(), f.h_score.data(),
                                      nullptr);
        }
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(sd.moves, f.h_moves[s].get(), (size_t)cnt * sizeof(oaz_move), hipMemcpyHostToDevice, sd.st));
        break;
    }
    }
    sd.calls++;
    HIP_TRY(launch_apply(v, sd, cnt));
    HIP_TRY(hipEventRecord(f.done[s], sd.st));
    HIP_TRY(hipStreamWaitEvent(f.route, f.done[s], 0));
    return 0;
}

// gm (slots mode): finished slots are harvested and refilled before every route. ss (optional): the rounds' counts.
int play(Fight& f, const arena::Slots& v, Side side[2], uint32_t* d_counts, const arena::Games* gm,
         oaz_arena_slots_stats* ss) {
    const bool shared = side[1].staged != nullptr;
    for (;;) {
        arena::SideBuf b1 = side[1].buf;
        if (shared) b1.roots = side[1].staged;
        if (gm) {
            hipLaunchKernelGGL(arena::k_arena_refill, dim3(1), dim3(arena::kRouteThreads), 0, f.route, v, *gm);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(arena::k_arena_route, dim3(1), dim3(arena::kRouteThreads), 0, f.route, v, side[0].buf, b1, d_counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(f.counts.get(), d_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, f.route));
        HIP_TRY(hipStreamSynchronize(f.route));
        const uint32_t cnt[2] = {f.counts[0], f.counts[1]};
        if (cnt[0] == 0 && cnt[1] == 0) return 0;
        for (int s = 0; s < 2; ++s)
            if (cnt[s] > side[s].buf.cap)
                return oaz_set_err(OAZ_ERR_CAPACITY, "arena: %u roots for a side sized for %u", cnt[s], side[s].buf.cap);
        if (ss) {
            ss->rounds++;
            for (int s = 0; s < 2; ++s) {
                ss->searches[s] += cnt[s] != 0;
                if (cnt[s] > ss->max_batch[s]) ss->max_batch[s] = cnt[s];
            }
        }
        // the sides whose work is only enqueued first, so a blocking side's search runs beside them
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < 2; ++s)
                if (cnt[s] && side[s].blocking() == (pass == 1))
                    if (int rc = side_ply(f, v, side[s], s, cnt[s])) return rc;
    }
}

// Both entry points. slots == 0 is the lock-step fight: one slot per game and nothing beyond what it always
// enqueued. Otherwise min(slots, game_amnt) slots, the per-game arrays and a refill before every route.
int fight_on(const oaz_arena_config* cfg, int32_t slots, const oaz_arena_agent* agent, const oaz_arena_agent* opponent,
             double agent_rating, double opponent_rating, oaz_fight_stats* stats, uint8_t* results, int32_t* plies,
             double* history, oaz_arena_slots_stats* ss) {
    if (int rc = check_arena_config(cfg)) return rc;
    if (!stats) return oaz_set_err(OAZ_ERR_ARG, "arena: null stats");
    const bool pooled = slots > 0;
    const int n = cfg->game_amnt;                   // games
    const int m = pooled && slots < n ? slots : n;  // slots
    if (ss) {
        memset(ss, 0, sizeof(*ss));
        ss->slots = (uint32_t)m;
    }
    std::vector<oaz_state> start;
    int32_t need[2] = {0, 0};
    initial_states(cfg, &start, need);
    if (m < n) need[0] = need[1] = m;  // (oaz_arena_slots_capacity)
    Side side[2];
    if (int rc = check_side("agent", agent, cfg, need[0], &side[0])) return rc;
    if (int rc = check_side("opponent", opponent, cfg, need[1], &side[1])) return rc;
    if (n == 0) return oaz_fight_stats_fold(nullptr, 0, agent_rating, opponent_rating, stats, history);
    if (int rc = oaz_check_device("arena", cfg->device)) return rc;
    OAZ_ON_DEVICE(cfg->device);

    Fight f;
    if (int rc = f.route.create()) return rc;
    if (int rc = f.counts.alloc(2)) return rc;
    const bool shared = side[0].ag.kind == OAZ_AGENT_ALPHAZERO && side[1].ag.kind == OAZ_AGENT_ALPHAZERO &&
                        side[0].ag.engine == side[1].ag.engine;
    arena::Slots v{};
    v.n = (uint32_t)m;
    arena::Games gm{};
    gm.n = (uint32_t)n;
    gm.max_plies = cfg->max_plies;
    uint32_t* d_counts = nullptr;
    auto carve = [&](Carver c) {
        v.state = c.take<oaz_state>(m);
        v.game = c.take<uint64_t>(m);
        v.plies = c.take<int32_t>(m);
        v.budget = c.take<int32_t>(m);
        v.passes = c.take<uint32_t>(m);
        v.progress = c.take<uint8_t>(m);
        v.active = c.take<uint8_t>(m);
        d_counts = c.take<uint32_t>(2);
        if (pooled) {
            gm.start = c.take<oaz_state>(n);
            gm.progress = c.take<uint8_t>(n);
            gm.plies = c.take<int32_t>(n);
            gm.passes = c.take<uint32_t>(n);
            gm.next = c.take<uint32_t>(1);
        }
        for (int s = 0; s < 2; ++s) {
            Side& sd = side[s];
            const bool az = sd.ag.kind == OAZ_AGENT_ALPHAZERO;
            sd.buf.cap = (uint32_t)need[s];
            sd.buf.idx = c.take<uint32_t>(need[s]);
            sd.buf.roots = az ? sd.ev.roots : c.take<oaz_state>(need[s]);
            sd.moves = az ? sd.ev.moves : c.take<oaz_move>(need[s]);
            sd.staged = (s == 1 && shared) ? c.take<oaz_state>(need[s]) : nullptr;
        }
        return c.off;
    };
    if (int rc = f.dev.alloc(carve(Carver{nullptr}))) return rc;
    carve(Carver{f.dev});
    for (int s = 0; s < 2; ++s) {
        Side& sd = side[s];
        if (int rc = f.done[s].create()) return rc;
        if (sd.ag.kind == OAZ_AGENT_ALPHAZERO) {
            sd.st = sd.ev.stream;
            continue;
        }
        if (int rc = f.side_st[s].create()) return rc;
        sd.st = f.side_st[s];
        if (sd.blocking()) {
            if (int rc = f.h_roots[s].alloc((size_t)need[s])) return rc;
            if (int rc = f.h_moves[s].alloc((size_t)need[s])) return rc;
        }
    }

    // every stream the fight used is waited for before a buffer goes, whatever happened
    auto drain = [&]() {
        hipError_t e = f.route.sync();
        for (int s = 0; s < 2; ++s) {
            const hipError_t es = hipStreamSynchronize(side[s].st);
            if (e == hipSuccess) e = es;
        }
        return e;
    };
    std::vector<uint64_t> ids((size_t)m);
    for (int k = 0; k < m; ++k) ids[(size_t)k] = (uint64_t)k;
    std::vector<uint8_t> h_progress((size_t)n);
    std::vector<int32_t> h_plies((size_t)n);
    std::vector<uint32_t> h_passes((size_t)n);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(v.state, start.data(), (size_t)m * sizeof(oaz_state), hipMemcpyHostToDevice, f.route));
        HIP_TRY(hipMemcpyAsync(v.game, ids.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, f.route));
        HIP_TRY(hipMemsetAsync(v.plies, 0, (size_t)m * 4, f.route));
        HIP_TRY(hipMemsetAsync(v.passes, 0, (size_t)m * 4, f.route));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)v.budget, cfg->max_plies, (size_t)m, f.route));
        HIP_TRY(hipMemsetAsync(v.progress, OAZ_IN_PROGRESS, (size_t)m, f.route));
        HIP_TRY(hipMemsetAsync(v.active, 1, (size_t)m, f.route));
        if (pooled) {  // slot i holds game i; the first game not dealt is m
            HIP_TRY(hipMemcpyAsync(const_cast<oaz_state*>(gm.start), start.data(), (size_t)n * sizeof(oaz_state),
                                   hipMemcpyHostToDevice, f.route));
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)gm.next, m, 1, f.route));
        }
        // the engines' streams may still run earlier work that reads their root buffers
        for (int s = 0; s < 2; ++s)
            if (side[s].ag.kind == OAZ_AGENT_ALPHAZERO) HIP_TRY(hipStreamSynchronize(side[s].st));
        if (int rc = play(f, v, side, d_counts, pooled ? &gm : nullptr, ss)) return rc;
        // (slots mode: the last refill, before the route that found no root, stored the last results)
        HIP_TRY(hipMemcpyAsync(h_progress.data(), pooled ? gm.progress : v.progress, (size_t)n, hipMemcpyDeviceToHost, f.route));
        HIP_TRY(hipMemcpyAsync(h_plies.data(), pooled ? gm.plies : v.plies, (size_t)n * 4, hipMemcpyDeviceToHost, f.route));
        HIP_TRY(hipMemcpyAsync(h_passes.data(), pooled ? gm.passes : v.passes, (size_t)n * 4, hipMemcpyDeviceToHost, f.route));
        return 0;
    };
    const int rc = run();
    const hipError_t de = drain();
    if (rc) return rc;
    HIP_TRY(de);

    if (int rc2 = oaz_fight_stats_fold(h_progress.data(), n, agent_rating, opponent_rating, stats, history)) return rc2;
    for (int k = 0; k < n; ++k) {
        stats->plies_total += (uint64_t)h_plies[(size_t)k];
        stats->passes += h_passes[(size_t)k];
        if (results) results[k] = h_progress[(size_t)k];
        if (plies) plies[k] = h_plies[(size_t)k];
    }
    return 0;
}

}  // namespace

extern "C" int oaz_arena_fight(const oaz_arena_config* cfg, const oaz_arena_agent* agent, const oaz_arena_agent* opponent,
                               double agent_rating, double opponent_rating, oaz_fight_stats* stats, uint8_t* results,
                               int32_t* plies, double* history) {
    return fight_on(cfg, 0, agent, opponent, agent_rating, opponent_rating, stats, results, plies, history, nullptr);
}

extern "C" int oaz_arena_fight_slots(const oaz_arena_config* cfg, int32_t slots, const oaz_arena_agent* agent,
                                     const oaz_arena_agent* opponent, double agent_rating, double opponent_rating,
                                     oaz_fight_stats* stats, uint8_t* results, int32_t* plies, double* history,
                                     oaz_arena_slots_stats* slot_stats) {
    if (int rc = check_arena_config(cfg)) return rc;  // (before the slot count, as the lock-step entry reports them)
    if (slots < 1) return oaz_set_err(OAZ_ERR_ARG, "arena: slots %d", slots);
    return fight_on(cfg, slots, agent, opponent, agent_rating, opponent_rating, stats, results, plies, history, slot_stats);
}
