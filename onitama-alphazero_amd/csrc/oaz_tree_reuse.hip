// oaz_tree_reuse.hip — tree reuse (oaz_config.reuse_visits > 0): the played move's subtree becomes the next
// search's tree. tree_rebase re-roots a game's tree in place at a child of its root (the compaction stated in
// oaz_tree_rebase.h, one wave per game as the other tree kernels); k_selfplay_rebase applies it between two
// self-play plies in place of k_tree_reset, k_tree_advance for oaz_search_advance. Part of the oaz_gpu.hip
// translation unit (after oaz_kernels.hip, whose device helpers it uses); it changes no other kernel.
// Also here, as the other entry point that reads the trees of the last search: oaz_search_sample_moves
// (k_sample_moves), the self-play temperature rule's draw for a caller that plays its own games.
#include <string.h>

#include <vector>

#include "oaz_host.h"
#include "oaz_tree_rebase.h"

namespace oaz {

// A node's pad word holds, during tree_rebase only, the number of members below the node and in the top bit
// whether the node is one; the function leaves every pad of the old tree 0 again.
constexpr uint32_t kRbMember = 0x80000000u;
constexpr int kNodeWords = (int)(sizeof(oaz_node) / 4), kPadWord = 7;
static_assert(sizeof(oaz_node) == 32 && offsetof(oaz_node, pad) == 4 * kPadWord, "oaz_node layout");

// Between stores and loads of one wave to the same global addresses by different lanes (no other wave touches the
// game's tree during the kernel). What is relied on: (1) the compiler moves no load or store across this point
// (the fences, and the asm's memory clobber); (2) every vector memory operation the wave has issued is complete
// before the next one is issued: the explicit s_waitcnt vmcnt(0), which on gfx9 counts loads and stores alike, so
// nothing depends on whether the compiler gives a workgroup-scope fence a wait of its own; (3) the CU's vector
// L1 is write-through and a store updates or drops the line it hits, so a later load of the same CU never reads
// an older copy: no cache invalidate is needed (nor emitted at workgroup scope), as for the tree kernels' own
// backup-then-select hand-over inside a wave.
__device__ __forceinline__ void rb_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Re-roots the n-node tree T at its node c (a child of the root, 1 <= c < n), in place, on one wave; returns
// the new node count (wave-uniform). Two ascending sweeps over the 64-node chunks from c's on:
//   1. membership and ranks. c is a member; a member that is expanded marks its children block, which lies
//      above it, possibly in the same chunk, so a chunk's marking repeats until no new member shows up in it.
//      Then every node of the chunk gets its rank (members below it: the running count + the members in lower
//      lanes) into its pad word;
//   2. the copy. Every lane reads its node and, if expanded, the rank at its old `first`, then all lanes write:
//      a member to its rank (never above its old index, so only chunks already read are overwritten), and 0
//      to the pad word it read from. The node that lands at index 0 becomes a fresh search's root.
__device__ __forceinline__ uint32_t tree_rebase(oaz_node* T, uint32_t n, uint32_t c) {
    const int l = lane_id();
    const uint64_t below = (1ull << l) - 1ull;
    uint32_t* W = reinterpret_cast<uint32_t*>(T);
    const uint32_t base0 = c & ~63u;
    if (l == 0) W[(size_t)c * kNodeWords + kPadWord] = kRbMember;
    rb_fence();
    uint32_t count = 0;
    for (uint32_t base = base0; base < n; base += 64) {
        const uint32_t i = base + (uint32_t)l;
        const bool in = i >= c && i < n;
        uint32_t* pad = &W[(size_t)(in ? i : c) * kNodeWords + kPadWord];
        uint32_t first = 0, len = 0, mark = 0;
        if (in) {
            const uint4 b = reinterpret_cast<const uint4*>(T + i)[1];
            first = b.y;
            len = rebase::block_len((uint32_t)node_flags(b.z), (uint32_t)node_nch(b.z));
            mark = b.w;
        }
        uint64_t done = 0;  // the chunk's members whose blocks are marked (wave-uniform)
        for (;;) {
            const uint64_t todo = __ballot(in && (mark & kRbMember)) & ~done;
            if (!todo) break;
            bool again = false;  // a block reached into this chunk
            for (uint64_t m = todo; m; m &= m - 1) {
                const int j = __ffsll((unsigned long long)m) - 1;
                const uint32_t f = (uint32_t)__shfl((int)first, j), k = (uint32_t)__shfl((int)len, j);
                if ((uint32_t)l < k && f + (uint32_t)l < n) W[(size_t)(f + (uint32_t)l) * kNodeWords + kPadWord] = kRbMember;
                again = again || (k && f < base + 64);
            }
            done |= todo;
            rb_fence();  // the marks are in memory before this chunk, or a later one, reads them
            if (!again) break;
            if (in) mark = *pad;
        }
        if (in) *pad = (mark & kRbMember) | (count + (uint32_t)__popcll(done & below));
        count += (uint32_t)__popcll(done);
    }
    const uint32_t total = count;
    rb_fence();
    for (uint32_t base = base0; base < n; base += 64) {
        const uint32_t i = base + (uint32_t)l;
        const bool in = i >= c && i < n;
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
        if (in) {
            const uint4* q = reinterpret_cast<const uint4*>(T + i);
            a = q[0];
            b = q[1];
        }
        const bool member = in && (b.w & kRbMember);
        if (member && rebase::remaps_first((uint32_t)node_flags(b.z)))
            b.y = b.y < n ? W[(size_t)b.y * kNodeWords + kPadWord] & ~kRbMember : total;
        rb_fence();  // every lane of the chunk has read before any lane writes
        if (in) W[(size_t)i * kNodeWords + kPadWord] = 0u;
        if (member) {
            const uint32_t j = b.w & ~kRbMember;
            if (j == 0) {  // the new root
                const uint64_t pb = __builtin_bit_cast(uint64_t, rebase::kRootP);
                a.z = (uint32_t)pb;
                a.w = (uint32_t)(pb >> 32);
                b.z = (b.z & 0xFFFF0000u) | rebase::kRootMv;
            }
            b.w = 0u;
            uint4* q = reinterpret_cast<uint4*>(T + j);
            q[0] = a;
            q[1] = b;
        }
    }
    rb_fence();
    return total;
}

// Counters of oaz_reuse_stats, in its field order.
enum ReuseStat { RS_KEPT = 0, RS_FRESH, RS_VISITS, RS_NODES, RS_COUNT };

// The tree of game g for its next search (lane 0 writes the count): root child c's subtree, or a fresh root.
__device__ __forceinline__ void next_tree(const TreeView& t, uint32_t g, bool keep, uint32_t c, uint32_t n,
                                          uint32_t visits, bool counted, unsigned long long* cnt) {
    oaz_node* T = t.nodes + (size_t)g * t.cap;
    if (keep) {
        const uint32_t total = tree_rebase(T, n, c);
        if (lane_id() == 0) {
            t.n_nodes[g] = total;
            atomicAdd(&cnt[RS_KEPT], 1ull);
            atomicAdd(&cnt[RS_VISITS], (unsigned long long)visits);
            atomicAdd(&cnt[RS_NODES], (unsigned long long)total);
        }
    } else if (lane_id() == 0) {
        store_fresh_node(T, 1.0, 0);  // what k_tree_reset writes
        t.n_nodes[g] = 1;
        if (counted) atomicAdd(&cnt[RS_FRESH], 1ull);
    }
}

// Between two self-play plies, in place of k_tree_reset: a slot that goes on with the game of the previous ply
// (active, ply > 0, and `prev`: the trees are that ply's) keeps the subtree of the move k_selfplay_move played,
// root_pi_best's last maximum of N, when the keep rule holds; a won game has ended (ply 0). Every other slot
// (a new game, a staggered start, an inactive slot, a pass) gets a fresh root.
// kTemp (temperature_plies = temp_plies > 0): where the previous ply drew its move (ply - 1 < temp_plies), the
// played child is that draw, recomputed from (seed, game id, ply - 1) on the same tree, not the last maximum.
template <bool kTemp>
__global__ void __launch_bounds__(kBlock) k_selfplay_rebase(TreeView t, SlotView sv, int prev, int32_t sims_cap,
                                                            int32_t R, uint32_t temp_plies, unsigned long long* cnt) {
    const uint32_t g = wave_game();
    if (g >= t.G) return;
    const oaz_node* T = t.nodes + (size_t)g * t.cap;
    const bool playing = sv.active[g] == 1;
    const uint32_t n = min(t.n_nodes[g], t.cap);
    uint32_t c = 0, visits = 0;
    bool keep = false;
    if (prev && playing && sv.ply[g] > 0) {  // (wave-uniform)
        float pl;
        int best, K;
        uint32_t mv;
        root_pi_best(T, nullptr, pl, best, K, mv);
        if (kTemp && K > 0 && sv.ply[g] - 1 < temp_plies) {  // (wave-uniform)
            const int drawn = root_temperature_child(T, sv.seed, sv.game_id[g], sv.ply[g] - 1, mv);
            if (drawn >= 0) best = drawn;
        }
        if (K > 0) {
            const NodeRegs root = load_node(&T[0]);
            c = root.first + (uint32_t)best;
            if (c >= 1 && c < n) {
                const NodeRegs ch = load_node(&T[c]);
                visits = ch.N;
                keep = rebase::keeps((uint32_t)node_flags(root.misc), (uint32_t)node_flags(ch.misc), ch.N, false,
                                     sims_cap, R);
            }
        }
    }
    next_tree(t, g, keep, c, n, visits, playing, cnt);
}

// The root child of T that `m` names: its node index (>= 1); 0 for a pass the position accepts (from = to = 25
// with one of the mover's cards, at a root without a child); -1 for anything else.
__device__ __forceinline__ int advance_find(const oaz_node* T, uint32_t n, const oaz_state& s, oaz_move m) {
    const int l = lane_id();
    const NodeRegs root = load_node(&T[0]);
    const int K = (int)rebase::block_len((uint32_t)node_flags(root.misc), (uint32_t)node_nch(root.misc));
    if (m.from == 25 && m.to == 25) return (K == 0 && m.slot < 4 && (m.slot >> 1) == (s.to_move & 1)) ? 0 : -1;
    if (m.from > 24 || m.to > 24 || m.slot > 3 || m.piece > 1) return -1;
    const uint32_t want = pack_move(m.from, m.to, m.slot, m.piece);
    const uint32_t idx = root.first + (uint32_t)l;
    bool hit = false;
    if (l < K && idx < n) hit = (load_node(&T[idx]).misc & 0xFFFFu) == want;
    const uint64_t hits = __ballot(hit);
    return hits ? (int)(root.first + (uint32_t)(__ffsll((unsigned long long)hits) - 1)) : -1;
}

// oaz_search_advance, first kernel: what advance_find says of every game's move; nothing is changed.
__global__ void __launch_bounds__(kBlock) k_advance_check(TreeView t, const oaz_state* __restrict__ roots,
                                                          const oaz_move* __restrict__ moves, int32_t* code) {
    const uint32_t g = wave_game();
    if (g >= t.G) return;
    const oaz_state s = load_state(&roots[g]);
    const int c = advance_find(t.nodes + (size_t)g * t.cap, min(t.n_nodes[g], t.cap), s, moves[g]);
    if (lane_id() == 0) code[g] = c;
}

// oaz_search_advance, second kernel (every move was found valid): the resident root steps by the move (or
// passes: the card goes round, nothing moves, as k_arena_apply), the side to move flips, and the tree becomes
// the moved-to child's subtree when the keep rule holds, a fresh root otherwise. kept[g] = the kept child's N.
__global__ void __launch_bounds__(kBlock) k_tree_advance(TreeView t, oaz_state* roots, const oaz_move* __restrict__ moves,
                                                         int32_t sims_cap, int32_t R, int32_t* kept,
                                                         unsigned long long* cnt) {
    const uint32_t g = wave_game();
    if (g >= t.G) return;
    const oaz_node* T = t.nodes + (size_t)g * t.cap;
    const uint32_t n = min(t.n_nodes[g], t.cap);
    oaz_state s = load_state(&roots[g]);
    const oaz_move m = moves[g];
    const int c = advance_find(T, n, s, m);
    if (c < 0) return;
    bool keep = false;
    uint32_t visits = 0;
    if (c == 0) {
        state_rotate(s, m.slot & 3);
    } else {
        const int res = make_move(s, m.from, m.to, m.piece, m.slot, s.to_move & 1);
        const NodeRegs root = load_node(&T[0]), ch = load_node(&T[c]);
        visits = ch.N;
        keep = rebase::keeps((uint32_t)node_flags(root.misc), (uint32_t)node_flags(ch.misc), ch.N, is_win(res), sims_cap,
                             R);
    }
    s.to_move ^= 1;
    if (lane_id() == 0) {
        store_state(&roots[g], s);
        kept[g] = keep ? (int32_t)visits : 0;
    }
    next_tree(t, g, keep, (uint32_t)c, n, visits, true, cnt);
}

hipError_t launch_selfplay_rebase(const TreeView& t, const SlotView& s, int prev, int32_t sims_cap, int32_t R,
                                  uint32_t temp_plies, uint64_t* counters, hipStream_t st) {
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
    if (temp_plies == 0)
        hipLaunchKernelGGL(k_selfplay_rebase<false>, dim3(wave_grid(t.G)), dim3(kBlock), 0, st, t, s, prev, sims_cap, R,
                           0u, cnt);
    else
        hipLaunchKernelGGL(k_selfplay_rebase<true>, dim3(wave_grid(t.G)), dim3(kBlock), 0, st, t, s, prev, sims_cap, R,
                           temp_plies, cnt);
    return hipGetLastError();
}

// oaz_search_sample_moves: the move the temperature rule draws from game g's resident tree for (gids[g], plies[g]):
// the drawn child, the last maximum of the visits where no child has a visit, the pass of k_search_finalize (child
// -1) at a root without a child.
__global__ void __launch_bounds__(kBlock) k_sample_moves(TreeView t, const oaz_state* __restrict__ roots, uint64_t seed,
                                                         const uint64_t* __restrict__ gids,
                                                         const uint32_t* __restrict__ plies, oaz_move* out_moves,
                                                         int32_t* out_child) {
    const uint32_t g = wave_game();
    if (g >= t.G) return;
    const oaz_node* T = t.nodes + (size_t)g * t.cap;
    float pl;
    int best, K;
    uint32_t mv;
    root_pi_best(T, nullptr, pl, best, K, mv);
    if (K > 0) {
        uint32_t drawn_mv = 0;
        const int c = root_temperature_child(T, seed, gids[g], plies[g], drawn_mv);
        if (c >= 0) {
            best = c;
            mv = drawn_mv;
        }
    }
    if (lane_id() == 0) {
        oaz_move m;
        if (K == 0) {  // no legal move (Q6): pass with the mover's first card
            m.from = 25;
            m.to = 25;
            m.piece = 0;
            m.slot = (uint8_t)((roots[g].to_move & 1) ? 2 : 0);
        } else {
            m.from = (uint8_t)mv_from(mv);
            m.to = (uint8_t)mv_to(mv);
            m.piece = (uint8_t)mv_piece(mv);
            m.slot = (uint8_t)mv_slot(mv);
        }
        out_moves[g] = m;
        out_child[g] = K == 0 ? -1 : best;
    }
}

}  // namespace oaz

using namespace oaz;

static TreeView reuse_tree_view(const oaz_reuse_engine_view& v, uint32_t G) {
    TreeView t{};
    t.nodes = v.nodes;
    t.n_nodes = v.n_nodes;
    t.cap = v.cap;
    t.G = G;
    return t;
}

extern "C" int oaz_search_advance(oaz_engine* e, const oaz_move* moves, int G, int32_t* kept) {
    oaz_reuse_engine_view v;
    if (int rc = oaz_engine_reuse_view(e, &v)) return rc;
    if (!moves || G < 0) return oaz_set_err(OAZ_ERR_ARG, "search_advance: bad arguments");
    if (v.reuse_visits <= 0) return oaz_set_err(OAZ_ERR_STATE, "search_advance: the engine was made with reuse_visits = 0");
    if ((uint32_t)G > v.searched)
        return oaz_set_err(OAZ_ERR_STATE, "search_advance: G=%d, but the trees of %u games are the last search's", G,
                           v.searched);
    if (G == 0) return 0;
    OAZ_ON_DEVICE(v.device);
    const TreeView t = reuse_tree_view(v, (uint32_t)G);
    std::vector<int32_t> h((size_t)G);
    HIP_TRY(hipMemcpyAsync(v.moves, moves, (size_t)G * sizeof(oaz_move), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_advance_check, dim3(wave_grid((uint32_t)G)), dim3(kBlock), 0, v.stream, t, v.roots, v.moves, v.codes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), v.codes, (size_t)G * 4, hipMemcpyDeviceToHost, v.stream));
    HIP_TRY(hipStreamSynchronize(v.stream));
    for (int g = 0; g < G; ++g)
        if (h[(size_t)g] < 0)
            return oaz_set_err(OAZ_ERR_ARG, "search_advance: move %d (from %d to %d, card slot %d) is neither a child of its root nor an accepted pass",
                               g, moves[g].from, moves[g].to, moves[g].slot);
    hipLaunchKernelGGL(k_tree_advance, dim3(wave_grid((uint32_t)G)), dim3(kBlock), 0, v.stream, t, v.roots, v.moves,
                       v.sims_cap, v.reuse_visits, v.kept, reinterpret_cast<unsigned long long*>(v.counters));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), v.kept, (size_t)G * 4, hipMemcpyDeviceToHost, v.stream));
    HIP_TRY(hipStreamSynchronize(v.stream));
    int32_t most = 0;
    for (int g = 0; g < G; ++g) {
        most = h[(size_t)g] > most ? h[(size_t)g] : most;
        if (kept) kept[g] = h[(size_t)g];
    }
    return oaz_engine_reuse_advanced(e, G, most);
}

extern "C" int oaz_search_sample_moves(oaz_engine* e, int G, const uint64_t* game_ids, const uint32_t* plies,
                                       oaz_move* out_moves, int32_t* out_child) {
    oaz_reuse_engine_view v;
    if (int rc = oaz_engine_reuse_view(e, &v)) return rc;
    if (G < 0 || !game_ids || !plies || (!out_moves && !out_child))
        return oaz_set_err(OAZ_ERR_ARG, "search_sample_moves: bad arguments");
    if ((uint32_t)G > v.searched)
        return oaz_set_err(OAZ_ERR_STATE, "search_sample_moves: G=%d, but the trees of %u games are the last search's", G,
                           v.searched);
    if (G == 0) return 0;
    OAZ_ON_DEVICE(v.device);
    // per-call scratch (freed on return, after the stream is done with it): a driver's call per ply, not a hot path
    DevBuf<uint64_t> d_gid;
    DevBuf<uint32_t> d_ply;
    DevBuf<oaz_move> d_mv;
    DevBuf<int32_t> d_child;
    if (d_gid.alloc((size_t)G) || d_ply.alloc((size_t)G) || d_mv.alloc((size_t)G) || d_child.alloc((size_t)G)) return OAZ_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(d_gid, game_ids, (size_t)G * 8, hipMemcpyHostToDevice, v.stream));
    HIP_TRY(hipMemcpyAsync(d_ply, plies, (size_t)G * 4, hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_sample_moves, dim3(wave_grid((uint32_t)G)), dim3(kBlock), 0, v.stream,
                       reuse_tree_view(v, (uint32_t)G), v.roots, v.seed, d_gid.get(), d_ply.get(), d_mv.get(), d_child.get());
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && out_moves)
        err = hipMemcpyAsync(out_moves, d_mv, (size_t)G * sizeof(oaz_move), hipMemcpyDeviceToHost, v.stream);
    if (err == hipSuccess && out_child) err = hipMemcpyAsync(out_child, d_child, (size_t)G * 4, hipMemcpyDeviceToHost, v.stream);
    const hipError_t done = hipStreamSynchronize(v.stream);  // before the scratch is freed, whatever happened
    HIP_TRY(err);
    HIP_TRY(done);
    return 0;
}

extern "C" int oaz_reuse_stats_get(oaz_engine* e, oaz_reuse_stats* out) {
    oaz_reuse_engine_view v;
    if (int rc = oaz_engine_reuse_view(e, &v)) return rc;
    if (!out) return oaz_set_err(OAZ_ERR_ARG, "reuse_stats: null");
    memset(out, 0, sizeof(*out));
    if (v.reuse_visits <= 0) return 0;
    OAZ_ON_DEVICE(v.device);
    uint64_t c[RS_COUNT];
    HIP_TRY(hipMemcpyAsync(c, v.counters, sizeof(c), hipMemcpyDeviceToHost, v.stream));
    HIP_TRY(hipStreamSynchronize(v.stream));
    out->trees_kept = c[RS_KEPT];
    out->trees_fresh = c[RS_FRESH];
    out->visits_kept = c[RS_VISITS];
    out->nodes_kept = c[RS_NODES];
    return 0;
}
