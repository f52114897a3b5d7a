// oaz_alphabeta.hip — the reference's alpha-beta agent on gfx950:
// onitama-game/src/ai/alpha_beta/mod.rs:35-183 + evaluation.rs:24-110 (the evaluation body: oaz_device.h).
//
// generate_move (mod.rs:136-170) deepens iteratively, depth = 1 .. max_depth - 1, and carries nothing from
// one iteration to the next (no move ordering, no table): not cut by the clock, its answer is the one
// search to max_depth - 1 plies. That search runs here; oaz_alphabeta_search does not enforce search_time,
// oaz_alphabeta_generate_move (the split search further down, max_depth up to 8) runs the loop with its clock.
//
// One wave answers one root, one lane per root move: lane k makes the k-th root move (card slot, from, to
// ascending: generate_legal_moves, state.rs:323-378) and searches that child with the full window
// (i32::MIN, i32::MAX); the wave then takes the first child in move order with the best score (Red the
// maximum, Blue the minimum). The sequential root (mod.rs:70-126) chooses the same move and score: it hands a
// later child the window (best so far, +inf), a child whose value does not exceed the best so far returns a
// fail-soft bound that does not exceed it either and never replaces the best under the strict `>`, and a
// child whose value exceeds it returns that value exactly. Only the number of positions visited differs.
//
// Inside a child the search is the reference's, move for move: Red maximises and Blue minimises (no negation),
// best_score starts at i32::MIN / i32::MAX and is returned as it is by a node without a legal move, a move
// replaces the best only on strict improvement, a node is terminal only when the move into it returned
// RedWin / BlueWin, and a cut-off (`break 'br`) leaves the loop over the current card's moves only: the second
// card's moves are still searched, with the alpha and beta the first card left.
//
// A lane's search is iterative: the node being expanded lives in registers, its ancestors below the root
// child in an LDS stack of at most 3 frames (state, alpha, beta, best and the move cursor: card, from-square,
// remaining pieces, remaining targets), [frame][word][thread] so a wave's accesses are conflict-free. Moves
// come off the attack masks as the cursor advances; leaves (depth max_depth - 1, or a won move) are
// evaluated in place without a frame.
//
// Defined where the reference panics: a root without a legal move returns the pass move (from = to = 25,
// piece 0, slot = the mover's first card) with the untouched best_score, like oaz_pure_mcts_search; a root
// whose every child returns the sentinel returns its first legal move with it; max_depth < 2 is OAZ_ERR_ARG.
#include <hip/hip_runtime.h>

#include <string.h>

#include <chrono>
#include <vector>

#include "../../include/onitama_az.h"
#include "oaz_device.h"
#include "oaz_host.h"

using namespace oaz;

namespace ab {

__constant__ AttackTable c_att = make_attack_table();

constexpr int kMaxPlies = 5;               // max_depth <= 6
constexpr int kMaxFrames = kMaxPlies - 2;  // stacked nodes: depth 1 .. plies - 2
constexpr int kFrameWords = 12;
constexpr int kThreads = 256, kGamesPerBlock = kThreads / 64;
constexpr int kAttWords = 2 * 16 * 25;

struct Cursor {  // where a node's move loop stands: moves come in (card, from, to) order
    uint32_t pieces, targets;  // own pieces not yet moved with this card; targets left for the piece on `from`
    int from, card;            // card: 0, 1 = the mover's first / second card, 2 = no move left
};

struct Frame {
    oaz_state s;
    int32_t alpha, beta, best;
    Cursor c;
};

__device__ __forceinline__ uint32_t own_pieces(const oaz_state& s, int color) {
    return color ? (s.pawns[1] | s.kings[1]) : (s.pawns[0] | s.kings[0]);
}

__device__ __forceinline__ void frame_open(Frame& f, const oaz_state& s, int32_t alpha, int32_t beta) {
    const int color = s.to_move & 1;
    f.s = s;
    f.alpha = alpha;
    f.beta = beta;
    f.best = color == OAZ_RED ? INT32_MIN : INT32_MAX;
    f.c = Cursor{own_pieces(s, color), 0u, 0, 0};
}

// The node's next move (packed), false when it has none left.
__device__ __forceinline__ bool next_move(const oaz_state& s, const uint32_t* att, Cursor& c, uint32_t* mv) {
    const int color = s.to_move & 1, s0 = color ? 2 : 0;
    const uint32_t occ = own_pieces(s, color);
    while (c.targets == 0) {
        if (c.pieces == 0) {
            if (c.card >= 1) {
                c.card = 2;
                return false;
            }
            c.card = 1;
            c.pieces = occ;
            continue;
        }
        c.from = __clz(c.pieces);
        c.pieces &= ~sq_bit(c.from);
        c.targets = att[(color * 16 + (state_card(s, s0 + c.card) & 15)) * 25 + c.from] & ~occ;
    }
    const int to = __clz(c.targets);
    c.targets &= ~sq_bit(to);
    const uint32_t pawns = color ? s.pawns[1] : s.pawns[0];
    *mv = pack_move(c.from, to, s0 + c.card, (pawns & sq_bit(c.from)) ? OAZ_PAWN : OAZ_KING);
    return true;
}

// mod.rs:93-124: a child's score arrives at its parent. A cut-off ends the current card's moves.
__device__ __forceinline__ void take_score(Frame& f, int32_t score) {
    bool cut;
    if ((f.s.to_move & 1) == OAZ_RED) {
        if (score > f.best) f.best = score;
        cut = score >= f.beta;
        if (!cut) f.alpha = max(f.alpha, score);
    } else {
        if (score < f.best) f.best = score;
        cut = score <= f.alpha;
        if (!cut) f.beta = min(f.beta, score);
    }
    if (cut || f.alpha >= f.beta) f.c.pieces = f.c.targets = 0u;
}

__device__ __forceinline__ void frame_store(uint32_t* slot, const Frame& f) {  // slot: word 0 of this thread
    uint32_t w[6];
    __builtin_memcpy(w, &f.s, 24);
#pragma unroll
    for (int i = 0; i < 6; ++i) slot[i * kThreads] = w[i];
    slot[6 * kThreads] = (uint32_t)f.alpha;
    slot[7 * kThreads] = (uint32_t)f.beta;
    slot[8 * kThreads] = (uint32_t)f.best;
    slot[9 * kThreads] = f.c.pieces;
    slot[10 * kThreads] = f.c.targets;
    slot[11 * kThreads] = (uint32_t)f.c.from | ((uint32_t)f.c.card << 8);
}

__device__ __forceinline__ void frame_load(const uint32_t* slot, Frame& f) {
    uint32_t w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = slot[i * kThreads];
    __builtin_memcpy(&f.s, w, 24);
    f.alpha = (int32_t)slot[6 * kThreads];
    f.beta = (int32_t)slot[7 * kThreads];
    f.best = (int32_t)slot[8 * kThreads];
    f.c.pieces = slot[9 * kThreads];
    f.c.targets = slot[10 * kThreads];
    const uint32_t fc = slot[11 * kThreads];
    f.c.from = (int)(fc & 0xFFu);
    f.c.card = (int)(fc >> 8);
}

// alpha_beta(1, plies, i32::MIN, i32::MAX, child, Some(mr)): the score, and the positions visited in *positions.
__device__ __forceinline__ int32_t search_child(const oaz_state& child, int mr, int plies, const uint32_t* att,
                                                uint32_t* stack /* this thread's word 0 of frame 0 */,
                                                uint32_t* positions) {
    uint32_t n_pos = 1;
    if (plies <= 1 || is_win(mr)) {
        *positions = n_pos;
        return alphabeta_evaluate(child, child.to_move & 1, is_win(mr));
    }
    Frame cur;
    frame_open(cur, child, INT32_MIN, INT32_MAX);
    int d = 1;  // depth of cur; stacked: depths 1 .. d - 1 in frames 0 .. d - 2
    for (;;) {
        uint32_t m;
        if (next_move(cur.s, att, cur.c, &m)) {
            oaz_state c = cur.s;
            const int res = make_move_regs(c, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), c.to_move & 1);
            c.to_move ^= 1;
            ++n_pos;
            if (d + 1 >= plies || is_win(res)) {
                take_score(cur, alphabeta_evaluate(c, c.to_move & 1, is_win(res)));
            } else {  // d <= plies - 2 <= kMaxFrames: frame d - 1 exists
                frame_store(stack + (size_t)(d - 1) * kFrameWords * kThreads, cur);
                frame_open(cur, c, cur.alpha, cur.beta);
                ++d;
            }
        } else {
            const int32_t score = cur.best;
            if (d == 1) {
                *positions = n_pos;
                return score;
            }
            --d;
            frame_load(stack + (size_t)(d - 1) * kFrameWords * kThreads, cur);
            take_score(cur, score);
        }
    }
}

__device__ __forceinline__ int32_t wave_best(int32_t v, bool red) {  // max for Red, min for Blue, over the wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = red ? max(v, o) : min(v, o);
    }
    return v;
}

// Dynamic LDS: the attack table (kAttWords words), then plies - 2 frames of kFrameWords x kThreads words.
__global__ __launch_bounds__(kThreads) void k_alphabeta(const oaz_state* roots, int G, int plies, oaz_move* out_move,
                                                        int32_t* out_score, uint32_t* out_positions) {
    extern __shared__ uint32_t lds[];
    uint32_t* att = lds;
    for (int i = threadIdx.x; i < kAttWords; i += kThreads) att[i] = (&c_att.m[0][0][0])[i];
    __syncthreads();  // (the only barrier: every thread reaches it)
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kGamesPerBlock + (threadIdx.x >> 6);
    if (g >= G || plies < 1 || plies - 2 > kMaxFrames) return;  // (wave-uniform)
    const oaz_state root = roots[g];
    const bool red = (root.to_move & 1) == OAZ_RED;
    // lane k's root move: the k-th of the move loop (lanes past the move count have none)
    Cursor rc{own_pieces(root, root.to_move & 1), 0u, 0, 0};
    uint32_t m = 0;
    bool has = true;
    for (int k = 0; k <= lane && has; ++k) has = next_move(root, att, rc, &m);
    int32_t score = red ? INT32_MIN : INT32_MAX;  // the reduction's identity = the untouched best_score
    uint32_t n_pos = 0;
    if (has) {
        oaz_state c = root;
        const int res = make_move_regs(c, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), c.to_move & 1);
        c.to_move ^= 1;
        score = search_child(c, res, plies, att, lds + kAttWords + threadIdx.x, &n_pos);
    }
    // the first child in move order with the best score (strict improvement, mod.rs:99-102, 110-113); when
    // every child returned the sentinel that is the first legal move
    const int32_t best = wave_best(score, red);
    const unsigned long long movers = __ballot(has), winners = __ballot(has && score == best);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_pos += __shfl_xor(n_pos, off, 64);
    const int first = winners ? __ffsll((long long)winners) - 1 : 0;
    const uint32_t bm = __shfl(m, first, 64);
    if (lane == 0) {
        oaz_move mv;
        if (movers == 0) {  // no legal move: pass with the mover's first card
            mv.from = 25;
            mv.to = 25;
            mv.piece = 0;
            mv.slot = (uint8_t)(red ? 0 : 2);
        } else {
            mv.from = (uint8_t)mv_from(bm);
            mv.to = (uint8_t)mv_to(bm);
            mv.piece = (uint8_t)mv_piece(bm);
            mv.slot = (uint8_t)mv_slot(bm);
        }
        out_move[g] = mv;
        out_score[g] = best;
        out_positions[g] = n_pos + 1;  // + the root
    }
}

// ---- the split search (oaz_alphabeta_generate_move) ------------------------------------------------------
// k_alphabeta gives a root one wave and walks every root child serially: right for 65 536 roots, and at most
// ~19 busy lanes for one. Here the first S plies of a call's roots are laid out as levels of nodes (level 0 the
// roots, level l + 1 the children of level l in move order: a count pass, an exclusive scan and a fill pass,
// so the order is the move order on every run), every level-S node ("item") is searched by one lane with the
// full window and the plies that remain (search_child, as above), and the exact values are folded upwards
// level by level with the reference's strict `>` / `<` from the untouched sentinel. A full-window item returns
// its exact value, so every interior node gets the value the sequential search would compute with the full
// window there, and the root takes the first child in move order that holds the best one: the same move and
// score as k_alphabeta and the sequential search (the argument at the top of this file, applied S times).
// Only the number of positions visited differs: no bound travels between items.
constexpr int kDeepMaxPlies = 7;  // max_depth <= 8 (bin/tournament.rs:107-110)
constexpr int kMaxSplit = 3;
constexpr int kDeepMaxFrames = kDeepMaxPlies - 1 - 1;  // an item at level S >= 1 stacks plies - S - 1 frames
static_assert(sizeof(uint32_t) * (kAttWords + (size_t)kDeepMaxFrames * kFrameWords * kThreads) <= 65536,
              "the deepest item's frame stack fits a workgroup's 64 KB of LDS");
constexpr int kLevelThreads = 256, kScanThreads = 1024;
constexpr uint32_t kLeaf = 4u;  // Level::flags: the MoveResult of the move into the node | kLeaf

struct Level {        // the nodes of one depth, in move order
    oaz_state* s;
    int32_t* value;   // leaves: written by the fill pass; items: by the search; interior nodes: by the fold
    uint32_t* move;   // the move into the node (packed); unused at level 0
    uint8_t* flags;
    uint32_t* off;    // [n + 1]: node i's children are nodes off[i] .. off[i + 1] - 1 of the next level
    uint64_t* pos;    // positions visited in the node's subtree, the node included
};

// off[i] = the number of children of node i: none for a leaf, else its legal moves.
__global__ __launch_bounds__(kLevelThreads) void k_ab_count(Level cur, uint32_t n) {
    const uint32_t i = blockIdx.x * kLevelThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t cnt = 0;
    if (!(cur.flags[i] & kLeaf)) {
        const oaz_state s = cur.s[i];
        Cursor c{own_pieces(s, s.to_move & 1), 0u, 0, 0};
        uint32_t m;
        while (next_move(s, &c_att.m[0][0][0], c, &m)) ++cnt;
    }
    cur.off[i] = cnt;
}

// In place: off[i] = off[0] + .. + off[i - 1] for i <= n (off[n] = the next level's size). One workgroup: thread
// t sums the t-th run of ceil(n / kScanThreads) counts, the run totals are scanned in LDS, the run is rewritten.
__global__ __launch_bounds__(kScanThreads) void k_ab_scan(uint32_t* off, uint32_t n) {
    __shared__ uint32_t run[kScanThreads];
    const uint32_t per = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += off[i];
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {  // (Hillis-Steele, inclusive)
        const uint32_t add = threadIdx.x >= (uint32_t)d ? run[threadIdx.x - d] : 0u;
        __syncthreads();
        run[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t acc = run[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = off[i];
        off[i] = acc;
        acc += c;
    }
    if (threadIdx.x == kScanThreads - 1) off[n] = run[kScanThreads - 1];
}

// Node i's children into nxt at off[i] .., in move order. A child reached by a winning move, or at the
// iteration's last ply (`last`), is a leaf and is evaluated here (mod.rs:50-58).
__global__ __launch_bounds__(kLevelThreads) void k_ab_fill(Level cur, uint32_t n, Level nxt, uint32_t n_next, int last) {
    const uint32_t i = blockIdx.x * kLevelThreads + threadIdx.x;
    if (i >= n || (cur.flags[i] & kLeaf)) return;
    const oaz_state s = cur.s[i];
    Cursor c{own_pieces(s, s.to_move & 1), 0u, 0, 0};
    uint32_t m;
    const uint32_t end = min(cur.off[i + 1], n_next);
    for (uint32_t k = cur.off[i]; k < end && next_move(s, &c_att.m[0][0][0], c, &m); ++k) {
        oaz_state ch = s;
        const int res = make_move_regs(ch, mv_from(m), mv_to(m), mv_piece(m), mv_slot(m), ch.to_move & 1);
        ch.to_move ^= 1;
        const bool leaf = last || is_win(res);
        nxt.s[k] = ch;
        nxt.move[k] = m;
        nxt.flags[k] = (uint8_t)((uint32_t)res | (leaf ? kLeaf : 0u));
        if (leaf) {
            nxt.value[k] = alphabeta_evaluate(ch, ch.to_move & 1, is_win(res));
            nxt.pos[k] = 1;
        }
    }
}

// One lane per item: alpha_beta(depth of the item, ..) with the full window, `plies` = the plies below the
// item's parent (search_child's count: leaves at depth plies). Dynamic LDS as k_alphabeta's.
__global__ __launch_bounds__(kThreads) void k_ab_items(Level it, uint32_t n, int plies) {
    extern __shared__ uint32_t lds[];
    uint32_t* att = lds;
    for (int i = threadIdx.x; i < kAttWords; i += kThreads) att[i] = (&c_att.m[0][0][0])[i];
    __syncthreads();  // (the only barrier: every thread reaches it)
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || plies < 2 || plies - 2 > kDeepMaxFrames) return;
    const uint32_t fl = it.flags[i];
    if (fl & kLeaf) return;
    uint32_t n_pos = 0;
    it.value[i] = search_child(it.s[i], (int)(fl & 3u), plies, att, lds + kAttWords + threadIdx.x, &n_pos);
    it.pos[i] = n_pos;
}

// Node i's value from its children's (mod.rs:93-124 without the window: the children's values are exact):
// strict improvement from the untouched sentinel, so a node without children keeps the sentinel. At level 0
// (out_move given) the root's move is the first child in move order with the best value; the first legal move
// when every child holds the sentinel; the pass move without a legal move (as k_alphabeta).
__global__ __launch_bounds__(kLevelThreads) void k_ab_fold(Level cur, uint32_t n, Level nxt, uint32_t n_next,
                                                            oaz_move* out_move, int32_t* out_score,
                                                            uint64_t* out_positions) {
    const uint32_t i = blockIdx.x * kLevelThreads + threadIdx.x;
    if (i >= n) return;
    if (cur.flags[i] & kLeaf) return;
    const bool red = (cur.s[i].to_move & 1) == OAZ_RED;
    int32_t best = red ? INT32_MIN : INT32_MAX;
    const uint32_t lo = min(cur.off[i], n_next), hi = min(cur.off[i + 1], n_next);
    uint32_t at = lo;
    uint64_t pos = 1;
    for (uint32_t k = lo; k < hi; ++k) {
        const int32_t v = nxt.value[k];
        if (red ? v > best : v < best) {
            best = v;
            at = k;
        }
        pos += nxt.pos[k];
    }
    cur.value[i] = best;
    cur.pos[i] = pos;
    if (!out_move) return;
    oaz_move mv;
    if (lo == hi) {  // no legal move: pass with the mover's first card
        mv.from = 25;
        mv.to = 25;
        mv.piece = 0;
        mv.slot = (uint8_t)(red ? 0 : 2);
    } else {
        const uint32_t bm = nxt.move[at];
        mv.from = (uint8_t)mv_from(bm);
        mv.to = (uint8_t)mv_to(bm);
        mv.piece = (uint8_t)mv_piece(bm);
        mv.slot = (uint8_t)mv_slot(bm);
    }
    out_move[i] = mv;
    out_score[i] = best;
    out_positions[i] = pos;
}

}  // namespace ab

extern "C" void oaz_alphabeta_config_default(oaz_alphabeta_config* c) {  // ai/alpha_beta/mod.rs:21-28
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_depth = 6;
    c->device = 0;
}

extern "C" int oaz_alphabeta_evaluate(const oaz_state* s, const uint8_t* move_result, int n, int32_t* out) {
    if (n < 0 || (n > 0 && (!s || !out))) return oaz_set_err(OAZ_ERR_ARG, "alphabeta_evaluate: null argument");
    for (int i = 0; i < n; ++i) {
        if ((s[i].to_move & ~1) || (move_result && move_result[i] > OAZ_IN_PROGRESS))
            return oaz_set_err(OAZ_ERR_ARG, "alphabeta_evaluate: position %d: to_move / move_result out of range", i);
        out[i] = alphabeta_evaluate(s[i], s[i].to_move, move_result && is_win(move_result[i]));
    }
    return 0;
}

static int check_roots(const oaz_state* roots, int G) {
    for (int g = 0; g < G; ++g)
        if (!oaz_root_ok(roots[g])) return oaz_set_err(OAZ_ERR_ARG, "alphabeta: root %d is not a valid state", g);
    return 0;
}

extern "C" int oaz_alphabeta_search(const oaz_state* roots, int G, const oaz_alphabeta_config* cfg, oaz_move* out_move,
                                    int32_t* out_score, oaz_alphabeta_stats* stats) {
    if (G < 0 || (G > 0 && (!roots || !out_move || !out_score)) || !cfg)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta: null argument");
    // mod.rs:161: max_depth < 2 runs no iteration and unwraps None; above 6 one lane would walk a root child's
    // whole subtree (1.8 M positions at max_depth 8): those depths are oaz_alphabeta_generate_move's, which
    // splits the tree over thousands of lanes
    if (cfg->max_depth < 2 || cfg->max_depth > ab::kMaxPlies + 1)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta: max_depth %d outside 2..%d", cfg->max_depth, ab::kMaxPlies + 1);
    if (int rc = check_roots(roots, G)) return rc;
    if (int rc = oaz_check_device("alphabeta", cfg->device)) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (G == 0) return 0;
    const int plies = cfg->max_depth - 1;
    const size_t lds_bytes = sizeof(uint32_t) * (ab::kAttWords + (size_t)(plies > 2 ? plies - 2 : 0) * ab::kFrameWords * ab::kThreads);
    // per call: roots, moves, scores, position counts (36 B per root); no kept workspace
    oaz_state* d_roots = nullptr;
    oaz_move* d_mv = nullptr;
    int32_t* d_sc = nullptr;
    uint32_t* d_pos = nullptr;
    auto carve = [&](Carver c) {
        d_roots = c.take<oaz_state>(G);
        d_mv = c.take<oaz_move>(G);
        d_sc = c.take<int32_t>(G);
        d_pos = c.take<uint32_t>(G);
        return c.off;
    };
    // on cfg->device, on a stream of its own (as oaz_pure_mcts_search): the null stream is not waited for, and
    // the calling thread's current device is restored on return. The stream is declared after the buffer: on
    // every return it is waited for before the buffer is freed (and before `pos` goes).
    OAZ_ON_DEVICE(cfg->device);
    std::vector<uint32_t> pos((size_t)G);
    DevBuf<char> buf;
    Stream sm;
    if (int rc = sm.create()) return rc;
    if (int rc = buf.alloc(carve(Carver{nullptr}))) return rc;
    carve(Carver{buf});
    HIP_TRY(hipMemcpyAsync(d_roots, roots, sizeof(oaz_state) * G, hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(ab::k_alphabeta, dim3((G + ab::kGamesPerBlock - 1) / ab::kGamesPerBlock), dim3(ab::kThreads),
                       lds_bytes, sm, d_roots, G, plies, d_mv, d_sc, d_pos);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sm));
    HIP_TRY(hipMemcpyAsync(out_move, d_mv, sizeof(oaz_move) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(out_score, d_sc, sizeof(int32_t) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(pos.data(), d_pos, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    if (stats)
        for (int g = 0; g < G; ++g) {
            stats->positions += pos[g];
            if (pos[g] > stats->max_positions_per_root) stats->max_positions_per_root = pos[g];
            stats->roots_without_move += out_move[g].from >= 25;
        }
    return 0;
}

// ---- oaz_alphabeta_generate_move: Agent::generate_move (mod.rs:136-170) with its clock -----------------------
extern "C" void oaz_alphabeta_agent_config_default(oaz_alphabeta_agent_config* c) {  // ai/alpha_beta/mod.rs:21-28
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_depth = 6;
    c->device = 0;
    c->search_time_ns = 1000000000;
    c->split = 0;
}

namespace {

// The levels an iteration of `plies` is split over for a call of G roots (split = 0), from two needs:
//   - lanes: one root yields ~12^S items (mid-game positions have 8-19 moves) and a launch wants tens of
//     thousands of them to fill the 256 CUs, so S is the smallest with G x 12^S >= 32 768 (G = 1 .. 18: 3,
//     G < 228: 2 or 3, G >= 2 731: 1). Every level costs pruning (1.7x, 3.8x, 5.9x the sequential search's
//     positions at S = 1, 2, 3 and max_depth 6), so a batch that fills the GPU at S = 1 stays there;
//   - a bounded launch: an item's serial walk grows ~12-fold per ply (20 616 positions at most over 4 plies,
//     1.8 M over 6 in the roots measured), so an item keeps at most 4 plies: S >= plies - 4 (max_depth 8: 3,
//     its longest item 63 970 positions; max_depth 7: 2).
// The larger of the two, at most kMaxSplit and plies - 1. Billions of items cannot follow from many roots:
// the roots of an iteration are searched kItemBudget / 20^S at a time (run_iteration's callers).
int auto_split(int G, int plies) {
    int s_fill = 1;
    for (double items = 12.0 * G; items < 32768.0 && s_fill < ab::kMaxSplit; items *= 12.0) ++s_fill;
    const int s_chain = plies - 4;
    return s_fill > s_chain ? s_fill : s_chain;
}

constexpr size_t kItemBudget = (size_t)1 << 22;  // items aimed at per launch (roots per launch: this / 20^S)
constexpr size_t kItemLimit = (size_t)1 << 27;   // nodes of one level at most (49 B each): OAZ_ERR_CAPACITY above

struct LevelBuf {  // one level's arrays in one grow-only allocation
    DevBuf<char> buf;
    ab::Level v{};
    static size_t carve(Carver c, size_t n, ab::Level* v) {
        v->s = c.take<oaz_state>(n);
        v->value = c.take<int32_t>(n);
        v->move = c.take<uint32_t>(n);
        v->flags = c.take<uint8_t>(n);
        v->off = c.take<uint32_t>(n + 1);
        v->pos = c.take<uint64_t>(n);
        return c.off;
    }
    // Room for n nodes. Growing frees the old allocation: the caller has synchronised the stream.
    int reserve(size_t n) {
        ab::Level none;
        if (int rc = buf.reserve(carve(Carver{nullptr}, n, &none))) return rc;
        carve(Carver{buf}, n, &v);
        return 0;
    }
};

inline dim3 blocks_of(uint32_t n, int threads) { return dim3((n + threads - 1) / threads); }

// One iteration over the gc roots at d_roots: their moves, scores and positions to out_*[0 .. gc). The stream is
// idle on return. *items += the level-S nodes.
int run_iteration(hipStream_t sm, LevelBuf* lv, const oaz_state* d_roots, uint32_t gc, int plies, int S,
                  oaz_move* out_move, int32_t* out_score, uint64_t* out_pos, uint64_t* items) {
    uint32_t n[ab::kMaxSplit + 1] = {gc, 0, 0, 0};
    if (int rc = lv[0].reserve(gc)) return rc;
    lv[0].v.s = const_cast<oaz_state*>(d_roots);  // level 0 reads the roots where they are
    HIP_TRY(hipMemsetAsync(lv[0].v.flags, OAZ_IN_PROGRESS, gc, sm));
    for (int l = 0; l < S; ++l) {
        if (n[l] > 0) {
            hipLaunchKernelGGL(ab::k_ab_count, blocks_of(n[l], ab::kLevelThreads), dim3(ab::kLevelThreads), 0, sm,
                               lv[l].v, n[l]);
            hipLaunchKernelGGL(ab::k_ab_scan, dim3(1), dim3(ab::kScanThreads), 0, sm, lv[l].v.off, n[l]);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&n[l + 1], lv[l].v.off + n[l], sizeof(uint32_t), hipMemcpyDeviceToHost, sm));
            HIP_TRY(hipStreamSynchronize(sm));
        }
        if (n[l + 1] > kItemLimit)
            return oaz_set_err(OAZ_ERR_CAPACITY, "alphabeta: %u nodes at level %d of a split search (at most %zu)",
                               n[l + 1], l + 1, kItemLimit);
        if (int rc = lv[l + 1].reserve(n[l + 1])) return rc;
        if (n[l + 1] > 0) {
            hipLaunchKernelGGL(ab::k_ab_fill, blocks_of(n[l], ab::kLevelThreads), dim3(ab::kLevelThreads), 0, sm,
                               lv[l].v, n[l], lv[l + 1].v, n[l + 1], l + 1 == plies ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
    }
    *items += n[S];
    const int below = plies - S + 1;  // search_child's plies: the item is its depth-1 node
    if (n[S] > 0 && below >= 2) {
        const size_t lds_bytes = sizeof(uint32_t) * (ab::kAttWords + (size_t)(below - 2) * ab::kFrameWords * ab::kThreads);
        hipLaunchKernelGGL(ab::k_ab_items, blocks_of(n[S], ab::kThreads), dim3(ab::kThreads), lds_bytes, sm, lv[S].v, n[S],
                           below);
        HIP_TRY(hipGetLastError());
    }
    for (int l = S - 1; l >= 0; --l) {
        if (n[l] == 0) continue;
        hipLaunchKernelGGL(ab::k_ab_fold, blocks_of(n[l], ab::kLevelThreads), dim3(ab::kLevelThreads), 0, sm, lv[l].v, n[l],
                           lv[l + 1].v, n[l + 1], l == 0 ? out_move : nullptr, out_score, out_pos);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(sm));
    return 0;
}

double ms_since(const std::chrono::steady_clock::time_point& t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" int oaz_alphabeta_generate_move(const oaz_state* roots, int G, const oaz_alphabeta_agent_config* cfg,
                                           oaz_move* out_move, int32_t* out_score, oaz_alphabeta_agent_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (G < 0 || (G > 0 && (!roots || !out_move || !out_score)) || !cfg)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta_generate_move: null argument");
    if (cfg->max_depth < 2 || cfg->max_depth > ab::kDeepMaxPlies + 1)  // mod.rs:161 below 2
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta_generate_move: max_depth %d outside 2..%d", cfg->max_depth,
                           ab::kDeepMaxPlies + 1);
    if (cfg->split < 0 || cfg->split > ab::kMaxSplit)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta_generate_move: split %d outside 0..%d", cfg->split, ab::kMaxSplit);
    if (cfg->search_time_ns < 0)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta_generate_move: search_time_ns %lld is negative",
                           (long long)cfg->search_time_ns);
    if (int rc = check_roots(roots, G)) return rc;
    if (int rc = oaz_check_device("alphabeta_generate_move", cfg->device)) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (G == 0) return 0;
    oaz_state* d_roots = nullptr;
    oaz_move* d_mv = nullptr;
    int32_t* d_sc = nullptr;
    uint64_t* d_pos = nullptr;
    auto carve = [&](Carver c) {
        d_roots = c.take<oaz_state>(G);
        d_mv = c.take<oaz_move>(G);
        d_sc = c.take<int32_t>(G);
        d_pos = c.take<uint64_t>(G);
        return c.off;
    };
    // as oaz_alphabeta_search: cfg->device, a stream of its own declared after the buffers (waited for before
    // they are freed), the calling thread's device restored on return
    OAZ_ON_DEVICE(cfg->device);
    std::vector<uint64_t> pos((size_t)G);
    DevBuf<char> buf;
    LevelBuf lv[ab::kMaxSplit + 1];
    Stream sm;
    if (int rc = sm.create()) return rc;
    if (int rc = buf.alloc(carve(Carver{nullptr}))) return rc;
    carve(Carver{buf});
    HIP_TRY(hipMemcpyAsync(d_roots, roots, sizeof(oaz_state) * G, hipMemcpyHostToDevice, sm));
    // mod.rs:145-156: iteration d starts while d < max_depth and the clock has not run out; a started one is
    // never abandoned, and the first always runs (the reference unwraps None instead). Without a clock only the
    // last iteration runs: nothing is carried from one to the next.
    const int last = cfg->max_depth - 1;
    int iterations = 0, plies = 0, S = 1;
    uint64_t items = 0;
    for (int d = cfg->search_time_ns > 0 ? 1 : last; d <= last; ++d) {
        if (iterations > 0 && ms_since(t0) * 1e6 >= (double)cfg->search_time_ns) break;
        S = cfg->split > 0 ? cfg->split : auto_split(G, d);
        S = S > d - 1 ? d - 1 : S;
        S = S < 1 ? 1 : S > ab::kMaxSplit ? ab::kMaxSplit : S;
        size_t per = kItemBudget;
        for (int l = 0; l < S; ++l) per /= 20;
        per = per < 1 ? 1 : per;
        items = 0;
        for (size_t g0 = 0; g0 < (size_t)G; g0 += per) {
            const uint32_t gc = (uint32_t)((size_t)G - g0 < per ? (size_t)G - g0 : per);
            if (int rc = run_iteration(sm, lv, d_roots + g0, gc, d, S, d_mv + g0, d_sc + g0, d_pos + g0, &items)) return rc;
        }
        plies = d;
        ++iterations;
    }
    HIP_TRY(hipMemcpyAsync(out_move, d_mv, sizeof(oaz_move) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(out_score, d_sc, sizeof(int32_t) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(pos.data(), d_pos, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    if (stats) {
        for (int g = 0; g < G; ++g) {
            stats->positions += pos[g];
            if (pos[g] > stats->max_positions_per_root) stats->max_positions_per_root = pos[g];
            stats->roots_without_move += out_move[g].from >= 25;
        }
        stats->items = items;
        stats->iterations = iterations;
        stats->plies = plies;
        stats->split = S;
        stats->elapsed_ms = ms_since(t0);
    }
    return 0;
}
