// oaz_pure_mcts.hip — the reference's pure-MCTS (random-rollout UCT) agent on gfx950
// (SURVEY.md 8f next #4): onitama-game/src/ai/mcts/mcts_arena.rs:56-264 + mod.rs:37-52.
//
// One thread per game runs the whole search (all playouts) in one launch: UCT selection in
// f32 with the last maximum winning ties (Iterator::max_by + f32::total_cmp, :147-156), expansion
// of a leaf once its visits exceed min_node_visits (:118-124, children in generate_all_legal_moves
// order), a uniformly random rollout to the end of the game with a random own card passed when
// no move exists (:190-230), and the +-1 reward backed up with a sign flip per level (:243-254).
// The final move is the most-visited root child (max_by_key, last maximum; :64-79) and the
// returned value its winrate.
//
// Defined where the reference is not: rollouts draw from a counter-based Philox stream keyed by
// (seed, game, playout) instead of thread_rng (draw = (u32 * n) >> 32); a rollout longer than
// rollout_cap plies scores 0 (the reference would keep playing); an expanded node without
// children (no legal move) is a leaf instead of a panic, and a root without children returns the
// pass move (from = to = 25, slot = the mover's first card) like oaz_search.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/onitama_az.h"
#include "oaz_device.h"
#include "oaz_host.h"

using namespace oaz;

namespace pm {

__constant__ AttackTable c_att = make_attack_table();

constexpr uint8_t kExpanded = 1, kTerminal = 2;
constexpr uint32_t kTag = 0x9C7A0000u;  // Philox counter word 2 for rollout draws

struct Rng {  // draw d of (game, playout): Philox(seed; game, playout, kTag, d / 4), word d % 4
    uint64_t seed;
    uint32_t game, playout, d;
    u32x4 buf;
    __device__ uint32_t next() {
        if ((d & 3) == 0) buf = philox(seed, game, playout, kTag, d >> 2);
        const uint32_t w = d & 3;
        ++d;
        return w == 0 ? buf.x : w == 1 ? buf.y : w == 2 ? buf.z : buf.w;
    }
    __device__ uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

// generate_all_legal_moves order (state.rs:301-378): card slot, from square, to square.
// Returns the number of moves; with k >= 0 also the k-th move (packed).
// (The state's colour- and slot-indexed fields are read through selects (state_card, make_move_regs): a
// runtime index into the struct put the whole state in scratch memory.)
__device__ __forceinline__ int movegen_kth(const oaz_state& s, int color, const uint32_t (*att)[25], int k,
                                          uint32_t* kth) {
    const uint32_t P = color ? s.pawns[1] : s.pawns[0], K = color ? s.kings[1] : s.kings[0], occ = P | K;
    const int s0 = color ? 2 : 0;
    int n = 0;
    for (int si = 0; si < 2; ++si) {
        const int card = state_card(s, s0 + si) & 15;
        uint32_t pieces = occ;
        while (pieces) {
            const int from = __clz(pieces);
            pieces &= ~sq_bit(from);
            uint32_t map = att[card][from] & ~occ;
            const int c = __popc(map);
            if (k >= n && k < n + c) {
                for (int j = k - n; j > 0; --j) map &= ~sq_bit(__clz(map));
                const int to = __clz(map);
                *kth = pack_move(from, to, s0 + si, (P & sq_bit(from)) ? OAZ_PAWN : OAZ_KING);
            }
            n += c;
        }
    }
    return n;
}

// A rollout ply's random move (mcts_arena.rs:190-230): the same move movegen_kth(s, color, att, k) returns for
// k = rng.below(n), n = the move count, from one pass over the mover's pieces (the masks of both cards kept in
// registers, then k located by the two cards' counts), not a counting pass and a second search pass. Returns n
// (0: no legal move; no draw is taken then, as before).
__device__ __forceinline__ int rollout_pick(const oaz_state& s, int color, const uint32_t (*att)[25], Rng& rng,
                                            uint32_t* mv) {
    const uint32_t P = color ? s.pawns[1] : s.pawns[0], K = color ? s.kings[1] : s.kings[0], occ = P | K;
    const int s0 = color ? 2 : 0;
    const uint32_t (*a0)[25] = att + (state_card(s, s0) & 15), (*a1)[25] = att + (state_card(s, s0 + 1) & 15);
    uint32_t m0[5], m1[5];
    int fr[5];
    int n0 = 0, n1 = 0;
    uint32_t pieces = occ;
#pragma unroll
    for (int i = 0; i < 5; ++i) {  // at most 5 pieces, in square order (generate_all_legal_moves)
        const int from = pieces ? __clz(pieces) : 0;
        fr[i] = from;
        m0[i] = pieces ? (*a0)[from] & ~occ : 0u;
        m1[i] = pieces ? (*a1)[from] & ~occ : 0u;
        n0 += __popc(m0[i]);
        n1 += __popc(m1[i]);
        pieces &= pieces ? ~sq_bit(from) : ~0u;
    }
    const int n = n0 + n1;
    if (n == 0) return 0;
    int k = (int)rng.below((uint32_t)n);
    const bool second = k >= n0;
    k -= second ? n0 : 0;
    uint32_t map = 0;
    int from = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint32_t m = second ? m1[i] : m0[i];
        const int c = __popc(m);
        if (!found && k < c) {
            map = m;
            from = fr[i];
            found = true;
        } else if (!found) {
            k -= c;
        }
    }
    for (; k > 0; --k) map &= ~sq_bit(__clz(map));
    *mv = pack_move(from, __clz(map), s0 + (second ? 1 : 0), (P & sq_bit(from)) ? OAZ_PAWN : OAZ_KING);
    return n;
}

__device__ __forceinline__ float reward_f(int result, int color) {  // mcts_arena.rs:233-241
    if (!is_win(result)) return 0.0f;
    return ((result == OAZ_RED_WIN) == (color == OAZ_RED)) ? 1.0f : -1.0f;
}

__device__ __forceinline__ int32_t total_key(float x) {  // f32::total_cmp as a signed integer order
    int32_t i = __float_as_int(x);
    return i ^ (int32_t)((uint32_t)(i >> 31) >> 1);
}

struct Params {
    int playouts, min_visits, rollout_cap;
    float c;
    uint64_t seed, game0;
    uint32_t cap;
};

#ifndef OAZ_PM_SELB
#define OAZ_PM_SELB 4
#endif
constexpr int kSelBatch = OAZ_PM_SELB;
#ifndef OAZ_PM_WPE
#define OAZ_PM_WPE 6
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OAZ_PM_WPE))) void k_pure_mcts(const oaz_state* roots, int G, Params p, const float* ln_tab,
                                                  oaz_pure_node* nodes, oaz_move* out_move, float* out_value,
                                                  uint64_t* stats /* [G][8] */) {
    __shared__ uint32_t att_s[2][16][25];
    for (int i = threadIdx.x; i < 2 * 16 * 25; i += blockDim.x) (&att_s[0][0][0])[i] = (&c_att.m[0][0][0])[i];
    __syncthreads();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    oaz_pure_node* T = nodes + (size_t)g * p.cap;
    const int root_color = roots[g].to_move & 1;
    T[0] = oaz_pure_node{0u, 0.0f, 0.0f, 0u, 0xFFFFFFFFu, 0, 0, 0};
    uint32_t n_nodes = 1;
    // the search's counters in LDS (the thread's own slots), out of the registers the walk and rollout need
    __shared__ uint64_t stl[5][64];
    uint64_t& st_plies = stl[0][threadIdx.x];
    uint64_t& st_pass = stl[1][threadIdx.x];
    uint64_t& st_exp = stl[2][threadIdx.x];
    uint64_t& st_capped = stl[3][threadIdx.x];
    uint64_t& st_over = stl[4][threadIdx.x];
    st_plies = st_pass = st_exp = st_capped = st_over = 0;
    for (int po = 0; po < p.playouts; ++po) {
        oaz_state s = roots[g];  // (reloaded per playout: an L2 hit, six registers fewer)
        uint32_t idx = 0;
        // 1. selection (mcts_arena.rs:100-116)
        while ((T[idx].flags & kExpanded) && !(T[idx].flags & kTerminal) && T[idx].nch) {
            const float lnN = ln_tab[T[idx].visits];
            const uint32_t first = T[idx].first, nch = T[idx].nch;
            uint32_t best = first;
            int32_t bk = INT32_MIN;
            // the children's (visits, winrate) kSelBatch at a time, all loads in flight before the fold (the
            // fold itself stays sequential in child order)
            for (uint32_t c0 = 0; c0 < nch; c0 += kSelBatch) {
                uint32_t vis[kSelBatch];
                float wr[kSelBatch];
#pragma unroll
                for (int j = 0; j < kSelBatch; ++j)
                    if (c0 + j < nch) {
                        vis[j] = T[first + c0 + j].visits;
                        wr[j] = T[first + c0 + j].winrate;
                    }
#pragma unroll
                for (int j = 0; j < kSelBatch; ++j)
                    if (c0 + j < nch) {
                        const float u = wr[j] + p.c * sqrtf(lnN / (float)vis[j]);
                        const int32_t k = total_key(u);
                        if (k >= bk) {  // max_by: the last maximum wins
                            bk = k;
                            best = first + c0 + j;
                        }
                    }
            }
            const uint32_t m = T[best].mv;
            const int color = s.to_move & 1;
            const int res = make_move_regs(s, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), color);
            s.to_move ^= 1;
            if (is_win(res)) T[best].flags |= kTerminal;
            idx = best;
        }
        // 2. expansion (mcts_arena.rs:118-124, 166-185)
        if (!(T[idx].flags & (kExpanded | kTerminal)) && T[idx].visits > (uint32_t)p.min_visits) {
            const int color = s.to_move & 1;
            const int n = movegen_kth(s, color, att_s[color], -1, nullptr);
            if (n_nodes + (uint32_t)n <= p.cap) {
                T[idx].first = n_nodes;
                T[idx].nch = (uint8_t)n;
                for (int k = 0; k < n; ++k) {
                    uint32_t m = 0;
                    movegen_kth(s, color, att_s[color], k, &m);
                    T[n_nodes + k] = oaz_pure_node{0u, 0.0f, 0.0f, 0u, idx, (uint16_t)m, 0, 0};
                }
                n_nodes += n;
                T[idx].flags |= kExpanded;
                ++st_exp;
            } else {
                ++st_over;  // capacity reached: the node stays a leaf
            }
        }
        // 3. simulation (mcts_arena.rs:188-231); reward colour = the colour that moved into idx
        const int reward_color = idx == 0 ? root_color : ((s.to_move & 1) ^ 1);
        Rng rng{p.seed, (uint32_t)(p.game0 + g), (uint32_t)po, 0u, {}};
        int mr = current_state(s);
        float r;
        if (is_win(mr)) {
            r = reward_f(mr, reward_color);
        } else {
            int color = s.to_move & 1, plies = 0;
            bool capped = false;
            while (!is_win(mr)) {
                if (plies >= p.rollout_cap) {
                    capped = true;
                    break;
                }
                uint32_t m = 0;
                const int n = rollout_pick(s, color, att_s[color], rng, &m);
                if (n == 0) {  // pass with a random own card (state.rs:139-142)
                    state_rotate(s, (color ? 2 : 0) + (int)rng.below(2));
                    color ^= 1;
                    ++st_pass;
                    ++plies;
                    continue;
                }
                mr = make_move_regs(s, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), color);
                color ^= 1;
                ++plies;
            }
            st_plies += plies;
            if (capped) {
                ++st_capped;
                r = 0.0f;
            } else {
                r = reward_f(mr, reward_color);
            }
        }
        // 4. backpropagation (mcts_arena.rs:243-254, MctsNode::update :361-365)
        for (uint32_t v = idx;;) {
            T[v].visits += 1;
            T[v].reward += r;
            T[v].winrate = T[v].reward / (float)T[v].visits;
            if (v == 0) break;
            v = T[v].parent;
            r = -r;
        }
    }
    // best root child by visits, last maximum (mcts_arena.rs:64-79)
    oaz_move mv;
    float value = 0.0f;
    if (T[0].nch == 0) {
        mv.from = 25;
        mv.to = 25;
        mv.piece = 0;
        mv.slot = (uint8_t)(root_color ? 2 : 0);
    } else {
        uint32_t best = T[0].first, bv = 0;
        for (uint32_t c = T[0].first; c < T[0].first + T[0].nch; ++c)
            if (T[c].visits >= bv) {
                bv = T[c].visits;
                best = c;
            }
        const uint32_t m = T[best].mv;
        mv.from = (uint8_t)mv_from(m);
        mv.to = (uint8_t)mv_to(m);
        mv.piece = (uint8_t)mv_piece(m);
        mv.slot = (uint8_t)mv_slot(m);
        value = T[best].winrate;
    }
    out_move[g] = mv;
    out_value[g] = value;
    uint64_t* st = stats + (size_t)g * 8;
    st[0] = (uint64_t)p.playouts;
    st[1] = st_exp;
    st[2] = st_plies;
    st[3] = st_pass;
    st[4] = st_capped;
    st[5] = n_nodes;
    st[6] = st_over;
    st[7] = 0;
}

// k_pure_mcts with the search's parameters per lane (oaz_pure_mcts_search_each): root g searches with par[g]'s
// playouts, min_node_visits and c on par[g]'s rollout stream, in its own slice [tree_off[g], tree_off[g + 1]) of
// the packed trees. The playout is k_pure_mcts's, statement for statement, but for two things:
//  - a UCT value that is NaN (0 * inf at c = 0 for an unvisited child) is ordered as the x86 default NaN
//    0xFFC00000, the smallest key of f32::total_cmp, whatever sign the GPU's multiplier gives it: that is the
//    value the reference's and the oracle's arithmetic produce;
//  - with the clock on, playout po >= floor starts only while the device's constant-rate clock is below the
//    lane's deadline (mcts_arena.rs:56-62: `while now.elapsed() < search_time && playouts < max_playouts`); the
//    first floor = min(playouts, min_visits + 2) playouts always run, so the root is expanded when it can be.
// A wave runs as long as its longest lane. Occupancy is not what bounds a launch of a few thousand roots, so
// the kernel takes the registers it needs to stay out of scratch memory.
struct EachParams {
    int rollout_cap, clock_on;
    uint64_t seed, ticks;
};

constexpr int32_t kNanKey = (int32_t)0x803FFFFFu;  // total_key of 0xFFC00000

#ifndef OAZ_PM_EACH_WPE
#define OAZ_PM_EACH_WPE 5
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OAZ_PM_EACH_WPE))) void k_pure_mcts_each(
    const oaz_state* roots, const oaz_pure_mcts_root* par, const uint64_t* tree_off, int G, EachParams p,
    const float* ln_tab, oaz_pure_node* nodes, oaz_move* out_move, float* out_value, int32_t* out_playouts,
    uint64_t* stats /* [G][8] */) {
    __shared__ uint32_t att_s[2][16][25];
    for (int i = threadIdx.x; i < 2 * 16 * 25; i += blockDim.x) (&att_s[0][0][0])[i] = (&c_att.m[0][0][0])[i];
    __syncthreads();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    oaz_pure_node* T = nodes + tree_off[g];
    const uint32_t cap = (uint32_t)(tree_off[g + 1] - tree_off[g]);
    const int playouts = par[g].max_playouts, min_visits = par[g].min_node_visits;
    const float c = par[g].exploration_c;
    const uint32_t stream = (uint32_t)par[g].stream;
    const int floor_po = min_visits >= playouts - 2 ? playouts : min_visits + 2;
    const uint64_t deadline = p.clock_on ? (uint64_t)wall_clock64() + p.ticks : 0;
    const int root_color = roots[g].to_move & 1;
    T[0] = oaz_pure_node{0u, 0.0f, 0.0f, 0u, 0xFFFFFFFFu, 0, 0, 0};
    uint32_t n_nodes = 1;
    __shared__ uint64_t stl[5][64];
    uint64_t& st_plies = stl[0][threadIdx.x];
    uint64_t& st_pass = stl[1][threadIdx.x];
    uint64_t& st_exp = stl[2][threadIdx.x];
    uint64_t& st_capped = stl[3][threadIdx.x];
    uint64_t& st_over = stl[4][threadIdx.x];
    st_plies = st_pass = st_exp = st_capped = st_over = 0;
    int po = 0;
    for (; po < playouts; ++po) {
        if (p.clock_on && po >= floor_po && (uint64_t)wall_clock64() >= deadline) break;
        oaz_state s = roots[g];
        uint32_t idx = 0;
        // 1. selection
        while ((T[idx].flags & kExpanded) && !(T[idx].flags & kTerminal) && T[idx].nch) {
            const float lnN = ln_tab[T[idx].visits];
            const uint32_t first = T[idx].first, nch = T[idx].nch;
            uint32_t best = first;
            int32_t bk = INT32_MIN;
            for (uint32_t c0 = 0; c0 < nch; c0 += kSelBatch) {
                uint32_t vis[kSelBatch];
                float wr[kSelBatch];
#pragma unroll
                for (int j = 0; j < kSelBatch; ++j)
                    if (c0 + j < nch) {
                        vis[j] = T[first + c0 + j].visits;
                        wr[j] = T[first + c0 + j].winrate;
                    }
#pragma unroll
                for (int j = 0; j < kSelBatch; ++j)
                    if (c0 + j < nch) {
                        const float u = wr[j] + c * sqrtf(lnN / (float)vis[j]);
                        const int32_t k = u != u ? kNanKey : total_key(u);
                        if (k >= bk) {  // max_by: the last maximum wins
                            bk = k;
                            best = first + c0 + j;
                        }
                    }
            }
            const uint32_t m = T[best].mv;
            const int color = s.to_move & 1;
            const int res = make_move_regs(s, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), color);
            s.to_move ^= 1;
            if (is_win(res)) T[best].flags |= kTerminal;
            idx = best;
        }
        // 2. expansion
        if (!(T[idx].flags & (kExpanded | kTerminal)) && T[idx].visits > (uint32_t)min_visits) {
            const int color = s.to_move & 1;
            const int n = movegen_kth(s, color, att_s[color], -1, nullptr);
            if (n_nodes + (uint32_t)n <= cap) {
                T[idx].first = n_nodes;
                T[idx].nch = (uint8_t)n;
                for (int k = 0; k < n; ++k) {
                    uint32_t m = 0;
                    movegen_kth(s, color, att_s[color], k, &m);
                    T[n_nodes + k] = oaz_pure_node{0u, 0.0f, 0.0f, 0u, idx, (uint16_t)m, 0, 0};
                }
                n_nodes += n;
                T[idx].flags |= kExpanded;
                ++st_exp;
            } else {
                ++st_over;  // capacity reached: the node stays a leaf
            }
        }
        // 3. simulation; reward colour = the colour that moved into idx
        const int reward_color = idx == 0 ? root_color : ((s.to_move & 1) ^ 1);
        Rng rng{p.seed, stream, (uint32_t)po, 0u, {}};
        int mr = current_state(s);
        float r;
        if (is_win(mr)) {
            r = reward_f(mr, reward_color);
        } else {
            int color = s.to_move & 1, plies = 0;
            bool capped = false;
            while (!is_win(mr)) {
                if (plies >= p.rollout_cap) {
                    capped = true;
                    break;
                }
                uint32_t m = 0;
                const int n = rollout_pick(s, color, att_s[color], rng, &m);
                if (n == 0) {  // pass with a random own card (state.rs:139-142)
                    state_rotate(s, (color ? 2 : 0) + (int)rng.below(2));
                    color ^= 1;
                    ++st_pass;
                    ++plies;
                    continue;
                }
                mr = make_move_regs(s, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), color);
                color ^= 1;
                ++plies;
            }
            st_plies += plies;
            if (capped) {
                ++st_capped;
                r = 0.0f;
            } else {
                r = reward_f(mr, reward_color);
            }
        }
        // 4. backpropagation
        for (uint32_t v = idx;;) {
            T[v].visits += 1;
            T[v].reward += r;
            T[v].winrate = T[v].reward / (float)T[v].visits;
            if (v == 0) break;
            v = T[v].parent;
            r = -r;
        }
    }
    // best root child by visits, last maximum (mcts_arena.rs:64-79)
    oaz_move mv;
    float value = 0.0f;
    if (T[0].nch == 0) {
        mv.from = 25;
        mv.to = 25;
        mv.piece = 0;
        mv.slot = (uint8_t)(root_color ? 2 : 0);
    } else {
        uint32_t best = T[0].first, bv = 0;
        for (uint32_t ch = T[0].first; ch < T[0].first + T[0].nch; ++ch)
            if (T[ch].visits >= bv) {
                bv = T[ch].visits;
                best = ch;
            }
        const uint32_t m = T[best].mv;
        mv.from = (uint8_t)mv_from(m);
        mv.to = (uint8_t)mv_to(m);
        mv.piece = (uint8_t)mv_piece(m);
        mv.slot = (uint8_t)mv_slot(m);
        value = T[best].winrate;
    }
    out_move[g] = mv;
    out_value[g] = value;
    out_playouts[g] = po;
    uint64_t* st = stats + (size_t)g * 8;
    st[0] = (uint64_t)po;
    st[1] = st_exp;
    st[2] = st_plies;
    st[3] = st_pass;
    st[4] = st_capped;
    st[5] = n_nodes;
    st[6] = st_over;
    st[7] = 0;
}

}  // namespace pm

extern "C" void oaz_pure_mcts_config_default(oaz_pure_mcts_config* c) {  // ai/mcts/mod.rs:21-30
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_playouts = 5000;
    c->min_node_visits = 5;
    c->exploration_c = 1.41421354f;  // 2f32.sqrt()
    c->rollout_cap = 1000;
    c->seed = 20260101ull;
    c->game_id0 = 0;
}

// Nodes one search may allocate (0 for a negative max_playouts): every expanded node first collects
// min_node_visits + 1 playouts as a leaf, so a search expands at most playouts / (min_node_visits + 1) nodes, each
// with <= 40 children.
static size_t tree_capacity(int max_playouts, int min_node_visits) {
    if (max_playouts < 0) return 0;
    const size_t exp = (size_t)max_playouts / (size_t)(min_node_visits + 1) + 1;
    return 1 + 40 * exp;
}

extern "C" size_t oaz_pure_mcts_tree_capacity(const oaz_pure_mcts_config* c) {
    return c ? tree_capacity(c->max_playouts, c->min_node_visits) : 0;
}

extern "C" size_t oaz_pure_mcts_each_capacity(const oaz_pure_mcts_root* par, int G, size_t* offsets) {
    size_t total = 0;
    for (int g = 0; par && g < G; ++g) {
        if (offsets) offsets[g] = total;
        total += par[g].min_node_visits < 0 ? 0 : tree_capacity(par[g].max_playouts, par[g].min_node_visits);
    }
    if (offsets && par && G >= 0) offsets[G] = total;
    return total;
}

// The search's device buffers as one allocation, and the last one of each device kept for the next call: a
// 1 M-search launch's trees take 64 GB, and allocating and freeing that per call cost 0.02-1.9 s on top of a
// 0.42 s search depending on the box (bench.py --mode pure_mcts). A call finding the kept buffer in use (a
// concurrent search on the same device) allocates its own and frees it on return.
// oaz_pure_mcts_release_workspace returns a device's kept buffer.
namespace {
struct PureWorkspace {
    std::mutex mu;
    DevBuf<char> buf;  // grow-only
    bool busy = false;
};
constexpr int kPureMaxDevices = 64;
// never deleted: no hipFree while the HIP runtime unloads at process exit (oaz_host.h)
PureWorkspace* const g_pure_ws = new PureWorkspace[kPureMaxDevices];

// A search's hold on its workspace (on the calling thread's current device, which is `dev`): the device's kept
// buffer, handed back on return, or a buffer of its own, freed on return.
struct WorkspaceLease {
    PureWorkspace* kept = nullptr;
    DevBuf<char> own;
    char* p = nullptr;
    int acquire(int dev, size_t bytes) {
        PureWorkspace& w = g_pure_ws[dev];
        {
            std::lock_guard<std::mutex> lk(w.mu);
            if (!w.busy) {
                if (int rc = w.buf.reserve(bytes)) return rc;  // (not busy: no search uses the old buffer)
                w.busy = true;
                kept = &w;
                p = w.buf;
                return 0;
            }
        }
        if (int rc = own.alloc(bytes)) return rc;
        p = own;
        return 0;
    }
    ~WorkspaceLease() {
        if (!kept) return;
        std::lock_guard<std::mutex> lk(kept->mu);
        kept->busy = false;
    }
};
}  // namespace

extern "C" int oaz_pure_mcts_release_workspace(int device) {
    if (device < 0 || device >= kPureMaxDevices) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts: device %d", device);
    PureWorkspace& w = g_pure_ws[device];
    std::lock_guard<std::mutex> lk(w.mu);
    if (w.busy) return oaz_set_err(OAZ_ERR_STATE, "pure_mcts: the workspace of device %d is in use", device);
    if (w.buf) {
        DeviceScope dev_scope_(device);
        w.buf.reset();
    }
    return 0;
}

// ---- the two searches' common host side ---------------------------------------------------------------------
namespace {
// What an entry point has checked and asks run_search for. par, off and out_playouts are
// oaz_pure_mcts_search_each's (one search per root, bin/mcts_parameter_check.rs's sweep in one launch per ply)
// and null for oaz_pure_mcts_search.
struct SearchCall {
    const char* who = nullptr;  // the error messages' prefix
    int device = 0, G = 0, max_playouts = 0;  // max_playouts: the call's largest search
    int64_t search_time_ns = 0;
    const oaz_state* roots = nullptr;
    const oaz_pure_mcts_root* par = nullptr;
    const uint64_t* off = nullptr;  // [G + 1]: the packed trees' offsets
    size_t nodes = 0;               // all trees together
    oaz_move* out_move = nullptr;
    float* out_value = nullptr;
    int32_t* out_playouts = nullptr;
    oaz_pure_mcts_stats* stats = nullptr;
    bool trees = false;  // copy_trees enqueues copies
};

// The workspace's sections (par, off and po empty without SearchCall::par) and the clock's budget in ticks.
struct SearchBuffers {
    oaz_state* roots;
    oaz_pure_mcts_root* par;
    uint64_t *off, *st /* [G][8] */;
    float *ln, *val;
    oaz_move* mv;
    int32_t* po;
    oaz_pure_node* nodes;
    uint64_t ticks;
};

// Everything after the argument checks: the device, the ln table, the workspace (the device's kept buffer, shared
// by both searches), the uploads, launch(buffers, stream), the results and statistics, and the trees that
// copy_trees(device nodes, stream) enqueues.
template <class Launch, class CopyTrees>
int run_search(const SearchCall& c, Launch launch, CopyTrees copy_trees) {
    const int G = c.G;
    if (int rc = oaz_check_device(c.who, c.device)) return rc;
    if (c.device >= kPureMaxDevices) return oaz_set_err(OAZ_ERR_ARG, "%s: device %d unsupported", c.who, c.device);
    SearchBuffers d{};
    if (c.search_time_ns > 0) {  // the budget in ticks of the device's constant-rate clock (as oaz_config.search_time_ns)
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c.device) != hipSuccess || khz <= 0)
            return oaz_set_err(OAZ_ERR_HIP, "%s: search_time: the device reports no wall clock rate", c.who);
        d.ticks = oaz_budget_ticks(c.search_time_ns, khz, 9e18);
    }
    std::vector<float> ln((size_t)c.max_playouts + 2);  // sized by the call's largest search
    for (size_t n = 0; n < ln.size(); ++n) ln[n] = logf((float)n);  // (parent.visits as f32).ln()
    auto carve = [&](Carver k) {
        d.roots = k.take<oaz_state>(G);
        d.par = k.take<oaz_pure_mcts_root>(c.par ? G : 0);
        d.off = k.take<uint64_t>(c.par ? (size_t)G + 1 : 0);
        d.ln = k.take<float>(ln.size());
        d.val = k.take<float>(G);
        d.mv = k.take<oaz_move>(G);
        d.po = k.take<int32_t>(c.par ? G : 0);
        d.st = k.take<uint64_t>((size_t)8 * G);
        d.nodes = k.take<oaz_pure_node>(c.nodes);
        return k.off;
    };
    const size_t ws_bytes = carve(Carver{nullptr});
    // on c.device, on a stream of its own: a search on a worker thread neither lands on the thread's default
    // device nor waits for (or stalls) the engines searching on the same GPU meanwhile. The stream is declared
    // after the workspace: on every return it is waited for before the workspace goes back or is freed (and
    // before `st` goes).
    OAZ_ON_DEVICE(c.device);
    std::vector<uint64_t> st((size_t)G * 8);
    WorkspaceLease ws;
    Stream sm;
    if (int rc = sm.create()) return rc;
    if (int rc = ws.acquire(c.device, ws_bytes)) return rc;
    carve(Carver{ws.p});
    HIP_TRY(hipMemcpyAsync(d.roots, c.roots, sizeof(oaz_state) * G, hipMemcpyHostToDevice, sm));
    if (c.par) {
        HIP_TRY(hipMemcpyAsync(d.par, c.par, sizeof(oaz_pure_mcts_root) * G, hipMemcpyHostToDevice, sm));
        HIP_TRY(hipMemcpyAsync(d.off, c.off, sizeof(uint64_t) * ((size_t)G + 1), hipMemcpyHostToDevice, sm));
    }
    HIP_TRY(hipMemcpyAsync(d.ln, ln.data(), sizeof(float) * ln.size(), hipMemcpyHostToDevice, sm));
    launch(d, sm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sm));
    HIP_TRY(hipMemcpyAsync(c.out_move, d.mv, sizeof(oaz_move) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(c.out_value, d.val, sizeof(float) * G, hipMemcpyDeviceToHost, sm));
    if (c.out_playouts) HIP_TRY(hipMemcpyAsync(c.out_playouts, d.po, sizeof(int32_t) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(st.data(), d.st, sizeof(uint64_t) * st.size(), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    if (c.stats)  // (zeroed by the entry point)
        for (int g = 0; g < G; ++g) {
            const uint64_t* s = &st[(size_t)g * 8];
            c.stats->playouts += s[0];
            c.stats->expansions += s[1];
            c.stats->rollout_plies += s[2];
            c.stats->rollout_passes += s[3];
            c.stats->rollouts_capped += s[4];
            if (s[5] > c.stats->max_nodes) c.stats->max_nodes = s[5];
            c.stats->tree_full += s[6];
        }
    if (c.trees) {
        if (int rc = copy_trees(d.nodes, sm)) return rc;
        HIP_TRY(hipStreamSynchronize(sm));
    }
    return 0;
}
}  // namespace

// Both entry points make every OAZ_ERR_ARG check before the first device query (whether or not a GPU is there),
// and G == 0 returns before cfg->device is looked at.
extern "C" int oaz_pure_mcts_search(const oaz_state* roots, int G, const oaz_pure_mcts_config* cfg,
                                    oaz_move* out_move, float* out_value, oaz_pure_mcts_stats* stats,
                                    oaz_pure_node* tree_out, size_t tree_cap) {
    if (G < 0 || (G > 0 && (!roots || !out_move || !out_value)) || !cfg)
        return oaz_set_err(OAZ_ERR_ARG, "pure_mcts: null argument");
    if (cfg->max_playouts < 0 || cfg->min_node_visits < 0 || cfg->rollout_cap < 0)
        return oaz_set_err(OAZ_ERR_ARG, "pure_mcts: negative playouts / min_node_visits / rollout_cap");
    for (int g = 0; g < G; ++g)
        if (!oaz_root_ok(roots[g])) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts: root %d is not a valid state", g);
    if (stats) memset(stats, 0, sizeof(*stats));
    if (G == 0) return 0;
    const size_t cap = tree_capacity(cfg->max_playouts, cfg->min_node_visits);
    if (cap > 0xFFFFFFF0u) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts: tree capacity too large");
    const pm::Params p{cfg->max_playouts, cfg->min_node_visits, cfg->rollout_cap, cfg->exploration_c, cfg->seed,
                       cfg->game_id0, (uint32_t)cap};
    SearchCall c;
    c.who = "pure_mcts";
    c.device = cfg->device;
    c.G = G;
    c.max_playouts = cfg->max_playouts;
    c.roots = roots;
    c.nodes = cap * G;
    c.out_move = out_move;
    c.out_value = out_value;
    c.stats = stats;
    c.trees = tree_out && tree_cap;
    return run_search(
        c,
        [&](const SearchBuffers& d, hipStream_t sm) {
            hipLaunchKernelGGL(pm::k_pure_mcts, dim3((G + 63) / 64), dim3(64), 0, sm, d.roots, G, p, d.ln, d.nodes, d.mv,
                               d.val, d.st);
        },
        [&](const oaz_pure_node* d_nodes, hipStream_t sm) {
            for (int g = 0; g < G; ++g)
                HIP_TRY(hipMemcpyAsync(tree_out + (size_t)g * tree_cap, d_nodes + (size_t)g * cap,
                                       sizeof(oaz_pure_node) * (tree_cap < cap ? tree_cap : cap), hipMemcpyDeviceToHost, sm));
            return 0;
        });
}

extern "C" int oaz_pure_mcts_search_each(const oaz_state* roots, const oaz_pure_mcts_root* par, int G,
                                         const oaz_pure_mcts_each_config* cfg, oaz_move* out_move, float* out_value,
                                         int32_t* out_playouts, oaz_pure_mcts_stats* stats, oaz_pure_node* tree_out,
                                         const size_t* tree_offsets) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "the packed trees' offsets are 64-bit on both sides");
    if (G < 0 || (G > 0 && (!roots || !par || !out_move || !out_value)) || !cfg)
        return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: null argument");
    if (tree_out && !tree_offsets) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: tree_out without tree_offsets");
    if (cfg->rollout_cap < 0) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: negative rollout_cap");
    if (cfg->search_time_ns < 0) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: negative search_time_ns");
    int max_playouts = 0;
    for (int g = 0; g < G; ++g) {
        if (par[g].max_playouts < 0 || par[g].min_node_visits < 0)
            return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: root %d: negative max_playouts / min_node_visits", g);
        if (par[g].stream >> 32)
            return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: root %d: stream %llu is not below 2^32", g,
                               (unsigned long long)par[g].stream);
        if (!oaz_root_ok(roots[g])) return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: root %d is not a valid state", g);
        if (tree_capacity(par[g].max_playouts, par[g].min_node_visits) > 0xFFFFFFF0u)
            return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: root %d: tree capacity too large", g);
        if (tree_out && tree_offsets[g + 1] < tree_offsets[g])
            return oaz_set_err(OAZ_ERR_ARG, "pure_mcts_each: root %d: tree_offsets decrease", g);
        if (par[g].max_playouts > max_playouts) max_playouts = par[g].max_playouts;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (G == 0) return 0;
    std::vector<uint64_t> off((size_t)G + 1);
    const size_t total = oaz_pure_mcts_each_capacity(par, G, reinterpret_cast<size_t*>(off.data()));
    SearchCall c;
    c.who = "pure_mcts_each";
    c.device = cfg->device;
    c.G = G;
    c.max_playouts = max_playouts;
    c.search_time_ns = cfg->search_time_ns;
    c.roots = roots;
    c.par = par;
    c.off = off.data();
    c.nodes = total;
    c.out_move = out_move;
    c.out_value = out_value;
    c.out_playouts = out_playouts;
    c.stats = stats;
    c.trees = tree_out != nullptr;
    return run_search(
        c,
        [&](const SearchBuffers& d, hipStream_t sm) {
            const pm::EachParams p{cfg->rollout_cap, cfg->search_time_ns > 0 ? 1 : 0, cfg->seed, d.ticks};
            hipLaunchKernelGGL(pm::k_pure_mcts_each, dim3((G + 63) / 64), dim3(64), 0, sm, d.roots, d.par, d.off, G, p,
                               d.ln, d.nodes, d.mv, d.val, d.po, d.st);
        },
        [&](const oaz_pure_node* d_nodes, hipStream_t sm) {
            // root g's nodes go to tree_out + tree_offsets[g], as many as its slice there holds; with the offsets of
            // oaz_pure_mcts_each_capacity that is the packed device array as it stands
            bool same = true;
            for (int g = 0; g <= G && same; ++g) same = tree_offsets[g] == off[g];
            if (same) {
                HIP_TRY(hipMemcpyAsync(tree_out, d_nodes, sizeof(oaz_pure_node) * total, hipMemcpyDeviceToHost, sm));
                return 0;
            }
            for (int g = 0; g < G; ++g) {
                const size_t have = off[g + 1] - off[g], room = tree_offsets[g + 1] - tree_offsets[g];
                HIP_TRY(hipMemcpyAsync(tree_out + tree_offsets[g], d_nodes + off[g],
                                       sizeof(oaz_pure_node) * (room < have ? room : have), hipMemcpyDeviceToHost, sm));
            }
            return 0;
        });
}
