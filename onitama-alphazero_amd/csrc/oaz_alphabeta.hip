// oaz_alphabeta.hip — the reference's alpha-beta agent on gfx950:
// onitama-game/src/ai/alpha_beta/mod.rs:35-183 + evaluation.rs:24-110 (the evaluation body: oaz_device.h).
//
// generate_move (mod.rs:136-170) deepens iteratively, depth = 1 .. max_depth - 1, and carries nothing from
// one iteration to the next (no move ordering, no table): not cut by the clock, its answer is the one
// search to max_depth - 1 plies. That search runs here; search_time is not enforced.
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

extern "C" int oaz_alphabeta_search(const oaz_state* roots, int G, const oaz_alphabeta_config* cfg, oaz_move* out_move,
                                    int32_t* out_score, oaz_alphabeta_stats* stats) {
    if (G < 0 || (G > 0 && (!roots || !out_move || !out_score)) || !cfg)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta: null argument");
    // mod.rs:161: max_depth < 2 runs no iteration and unwraps None; above 6 is not opened yet (a depth-7
    // search is ~40x a depth-5 one, whose kernel time on a shared GPU nobody has measured)
    if (cfg->max_depth < 2 || cfg->max_depth > ab::kMaxPlies + 1)
        return oaz_set_err(OAZ_ERR_ARG, "alphabeta: max_depth %d outside 2..%d", cfg->max_depth, ab::kMaxPlies + 1);
    for (int g = 0; g < G; ++g)  // (bitboards hold squares 0..24 only: the kernel indexes the attack table by square)
        if ((roots[g].to_move & ~1) || (roots[g].cards[0] | roots[g].cards[1] | roots[g].cards[2] | roots[g].cards[3] |
                                        roots[g].cards[4]) > 15 ||
            ((roots[g].kings[0] | roots[g].kings[1] | roots[g].pawns[0] | roots[g].pawns[1]) & 0x7Fu))
            return oaz_set_err(OAZ_ERR_ARG, "alphabeta: root %d is not a valid state", g);
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
