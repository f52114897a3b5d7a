// oaz_search_par.hip — leaf-parallel search with virtual loss (oaz_config.leaf_batch = L, 1 <= L <= 16;
// DESIGN.md "Leaf-parallel search"): the whole search of a few roots in ONE launch, one workgroup per root as
// k_search_lat, but a network pass evaluates up to L leaves of the SAME tree as one 16-position tile (k_nn_h3's
// body, as k_search_grp runs it) where k_search_lat evaluates one.
//
// The rule, in rounds until done == sims:
//   collect  for j = 0 .. min(L, sims - done) - 1, in order: walk from the root as k_select does, on the
//            effective statistics n = N + v, q = n ? (W - (double)v) / (double)n : 0,
//            u = q + c_puct * P * (sqrt_tab[N_p + v_p] / (double)(n + 1)), v = the node's in-flight count
//            (oaz_node.pad, 0 outside a round). A walk that ends on a node that is neither expanded nor
//            terminal-flagged and already has v > 0 is discarded and closes the round; every other walk adds 1
//            to v along its path (root included) and records its path and leaf position as leaf j;
//   evaluate the m collected leaves as one tile (rows m .. 15 hold copies of row 0 and are not used);
//   back up  for j = 0 .. m - 1, in order: v -= 1 along path j, then the playout's expand / back up, unchanged
//            (expand_backup_seg_body on leaf j's records); done += m.
// With L = 1 this is the sequential search bit for bit (W - 0.0 == W). One walker wave (wave 0) runs the collect
// and the back up sequentially in j; all eight waves evaluate the tile.
//
// The tree, the paths and the leaf records stay in global memory (L2): the tile body and its fp16-range
// recompute use the kernel's whole LDS (H3Fallback::kLds, 157.7 KB of 160), which leaves no room for
// k_search_lat's LDS copy of the top of the tree beside them.
//
// Q7 search_time: thread 0 reads the device clock before every round after the first; a search stops only at a
// round boundary, sims_run[g] = done.
namespace oaz {

struct ParNode {  // a node with its in-flight count
    double W, P;
    uint32_t N, first, misc, v;
};
__device__ __forceinline__ ParNode par_load_node(const oaz_node* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    ParNode r;
    r.W = __builtin_bit_cast(double, ((uint64_t)a.y << 32) | a.x);
    r.P = __builtin_bit_cast(double, ((uint64_t)a.w << 32) | a.z);
    r.N = b.x;
    r.first = b.y;
    r.misc = b.z;
    r.v = b.w;
    return r;
}
__device__ __forceinline__ void par_fence() {  // the walker wave's own stores, visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The collect phase of one round on the walker wave (all 64 lanes; lane l holds child l, K <= 40 < 64, as
// lat_select_wide): up to `want` walks. t is the root's own view (G = 1; path / depth / leaf / leaf_state: leaf
// 0's records, leaf j's follow at j * pathcap, j, j, j). Returns the leaves collected (uniform); *disc = 1 when a
// discarded walk closed the round.
__device__ __noinline__ uint32_t par_collect(const TreeView& t, const oaz_state* root, const SearchParams& prm,
                                             uint32_t want, uint32_t* disc) {
    const int l = (int)(threadIdx.x & 63);
    oaz_node* T = t.nodes;
    uint32_t m = 0;
    *disc = 0;
    for (uint32_t j = 0; j < want; ++j) {
        uint32_t* path = t.path + (size_t)j * t.pathcap;
        oaz_state s = load_state(root);
        int color = s.to_move & 1;
        ParNode nd = par_load_node(T);
        uint32_t node = 0, depth = 0;
        if (l == 0) path[0] = 0;
        bool stuck = false;
        while ((node_flags(nd.misc) & 1) && !(node_flags(nd.misc) & 2)) {
            const int K = node_nch(nd.misc);
            if (K == 0) {  // reference would panic in select (Q6): stop here, treat as a leaf
                stuck = true;
                break;
            }
            ParNode ch;
            ch.W = 0.0;
            ch.P = 0.0;
            ch.N = 0;
            ch.first = 0;
            ch.misc = 0;
            ch.v = 0;
            if (l < K) ch = par_load_node(T + nd.first + l);
            const double sqn = t.sqrt_tab[nd.N + nd.v];  // N_p + v_p <= sims
            int64_t key = INT64_MIN;
            if (l < K) {
                const uint32_t n = ch.N + ch.v;
                const double q = n ? (ch.W - (double)ch.v) / (double)n : 0.0;
                const double sq = sqn / (double)(n + 1);
                const double u = q + prm.c_puct * ch.P * sq;  // mcts_arena.rs:204-207 on the effective statistics
                key = total_key(u);
            }
            int idx = l;
            seg_amax_step<0xB1>(key, idx);  // within each row of 16 lanes (every lane ends with its row's best)
            seg_amax_step<0x4E>(key, idx);
            seg_amax_step<0x141>(key, idx);
            seg_amax_step<0x140>(key, idx);
            int best = __builtin_amdgcn_readlane(idx, 0);
            int64_t bkey = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)key >> 32), 0) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)key, 0));
#pragma unroll
            for (int r = 1; r < 4; ++r) {  // rows hold ascending children: a tie goes to the later row
                const int64_t rk =
                    (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)key >> 32), 16 * r) << 32) |
                              (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)key, 16 * r));
                const int ri = __builtin_amdgcn_readlane(idx, 16 * r);
                if (rk > bkey || (rk == bkey && ri > best)) {
                    bkey = rk;
                    best = ri;
                }
            }
            ParNode c;  // (the walk reads only N, first, misc and v of the node it descends to)
            c.W = 0.0;
            c.P = 0.0;
            c.N = (uint32_t)__builtin_amdgcn_readlane((int)ch.N, best);
            c.first = (uint32_t)__builtin_amdgcn_readlane((int)ch.first, best);
            c.misc = (uint32_t)__builtin_amdgcn_readlane((int)ch.misc, best);
            c.v = (uint32_t)__builtin_amdgcn_readlane((int)ch.v, best);
            const uint32_t cidx = nd.first + (uint32_t)best;
            const int res = make_move_regs(s, mv_from(c.misc), mv_to(c.misc), mv_piece(c.misc), mv_slot(c.misc), color);
            color ^= 1;  // game_state.player_color.switch()
            if (is_win(res)) {
                c.misc |= 2u << 24;
                if (l == 0) *flags_ptr(T + cidx) = (uint8_t)(node_flags(c.misc));
            }
            ++depth;
            if (l == 0 && depth < t.pathcap) path[depth] = cidx;
            node = cidx;
            nd = c;
        }
        s.to_move = (uint8_t)color;
        if (!(node_flags(nd.misc) & 3) && nd.v > 0) {  // this leaf is already in flight: the round closes here
            *disc = 1;
            par_fence();  // (a terminal flag the walk set)
            break;
        }
        if (l == 0) {
            const bool need = leaf_needs_eval(nd.misc, s);
            store_state(t.leaf_state + j, s);
            t.leaf[j] = node;
            t.depth[j] = depth;
            t.stats[GS_SIMS] += 1;  // one writer: this lane
            t.stats[GS_DEPTH] += depth;
            t.stats[GS_EVALS] += need;
            if (stuck) t.stats[GS_STUCK] += 1;
        }
        par_fence();  // the path, written by lane 0
        const uint32_t plen = depth < t.pathcap ? depth : t.pathcap - 1;
        for (uint32_t k = (uint32_t)l; k <= plen; k += 64) T[path[k]].pad += 1;  // (a path's nodes are distinct)
        par_fence();
        ++m;
    }
    // the tile's unused rows: copies of row 0, so that no stale position enters the network pass
    if (l >= (int)m && l < nn::kSB && m > 0) t.leaf_state[l] = t.leaf_state[0];
    return m;
}

// The back up phase of one round on the walker wave: leaf j's in-flight counts come off its path, then the
// playout's own expand / back up runs on leaf j's records and evaluation row (segment 0 of the wave holds the
// game, the other segments idle, as in k_search_lat).
__device__ __noinline__ void par_backup(const TreeView& t, const oaz_state* root, const float* policy,
                                        const float* value, uint32_t m, float* sp) {
    const int l = (int)(threadIdx.x & 63);
    const uint32_t gs = l < 16 ? 0u : 1u;
    for (uint32_t j = 0; j < m; ++j) {
        TreeView tj = t;
        tj.path = t.path + (size_t)j * t.pathcap;
        tj.depth = t.depth + j;
        tj.leaf = t.leaf + j;
        tj.leaf_state = t.leaf_state + j;
        const uint32_t depth = *tj.depth;
        const uint32_t plen = depth < t.pathcap ? depth : t.pathcap - 1;
        for (uint32_t k = (uint32_t)l; k <= plen; k += 64) t.nodes[tj.path[k]].pad -= 1;
        par_fence();
        expand_backup_seg_body(tj, root, nullptr, policy + (size_t)j * 50, value + j, gs, sp, NodesGlobalRegs{});
        par_fence();
    }
}

// The per-root records of the leaf-parallel search (allocated with leaf_batch > 0 only): L paths, depths and
// leaf ids per root, and 16 leaf positions and evaluation rows per root (a whole tile each: rows L .. 15 are
// never used).
struct ParView {
    uint32_t* path;         // [G][L][pathcap]
    uint32_t* depth;        // [G][L]
    uint32_t* leaf;         // [G][L]
    oaz_state* leaf_state;  // [G][16]
    float* policy;          // [G][16][50]
    float* value;           // [G][16]
    uint64_t* lb_stats;     // [G][3] rounds, playouts, discarded walks of the search
    uint32_t L;
};

__global__ void __launch_bounds__(kLatThreads) k_search_par(TreeView t, ParView pv, const oaz_state* __restrict__ roots,
                                                            SearchParams prm, int sims, int hash_eval,
                                                            const float* __restrict__ blob, int blocks,
                                                            const float* __restrict__ xblob,
                                                            unsigned long long* __restrict__ fallback,
                                                            const uint64_t* __restrict__ deadline,
                                                            uint32_t* __restrict__ sims_run) {
    using C = H3Cfg<0>;
    __shared__ __attribute__((aligned(16))) float lds[H3Fallback<C>::kLds];
    __shared__ uint32_t round_m[2];  // the round's leaves, whether a discarded walk closed it
    const uint32_t g = blockIdx.x;
    if (g >= t.G) return;  // uniform over the workgroup
    const int tid = (int)threadIdx.x;
    const bool walker = (tid >> 6) == 0;
    const uint32_t L = pv.L;
    // the root's slice of the tree arrays (one game: index 0), the records leaf 0's
    TreeView tg = t;
    tg.nodes = t.nodes + (size_t)g * t.cap;
    tg.n_nodes = t.n_nodes + g;
    tg.path = pv.path + (size_t)g * L * t.pathcap;
    tg.depth = pv.depth + (size_t)g * L;
    tg.leaf = pv.leaf + (size_t)g * L;
    tg.leaf_state = pv.leaf_state + (size_t)g * nn::kSB;
    tg.stats = t.stats + (size_t)g * GS_COUNT;
    tg.need = nullptr;
    tg.slot = nullptr;
    tg.G = 1;
    const oaz_state* rg = roots + g;
    float* const pol = pv.policy + (size_t)g * nn::kSB * 50;
    float* const val = pv.value + (size_t)g * nn::kSB;
    float* const sp = lds + (tid >> 4) * 52;  // the segment's policy row (the network's LDS, free meanwhile)
    const int b0 = (int)g * nn::kSB;
    const uint64_t dl = deadline ? *deadline : 0;  // Q7 (null: no budget, exactly `sims` playouts)
    uint32_t done = 0, rounds = 0, discarded = 0;
    while (done < (uint32_t)sims) {
        if (deadline && rounds > 0 && __syncthreads_or(tid == 0 && (uint64_t)wall_clock64() >= dl)) break;
        if (walker) {
            const uint32_t left = (uint32_t)sims - done;
            uint32_t disc;
            const uint32_t mm = par_collect(tg, rg, prm, left < L ? left : L, &disc);
            if (tid == 0) {
                round_m[0] = mm;
                round_m[1] = disc;
            }
        }
        __syncthreads();  // the round's leaf positions
        const uint32_t m = round_m[0];
        discarded += round_m[1];
        if (hash_eval) {
            for (int k = tid; k < (int)m * 50; k += kLatThreads) {
                const int r = k / 50, e = k % 50;
                const uint64_t h = hash_state(load_state(&tg.leaf_state[r]));
                pol[(size_t)r * 50 + e] = hash_policy(h, e);
                if (e == 0) val[r] = hash_value(h);
            }
        } else {
            const TileSpan span{b0, b0 + (int)m, (int)t.G * nn::kSB};
            int opaque;  // 0, opaque to the compiler: no lane offset of the body is hoisted out of this loop
            asm volatile("v_mov_b32 %0, 0" : "=v"(opaque));
            bool ovf;
            if ((tid >> 8) == 0) {
                __builtin_amdgcn_s_setprio(1);
                ovf = nn_h3_body<C, C::GRP0>(pv.leaf_state, span, blob, blocks, pv.policy, pv.value, lds, opaque);
            } else {
                ovf = nn_h3_body<C, C::GRP1>(pv.leaf_state, span, blob, blocks, pv.policy, pv.value, lds, opaque);
            }
            using X = typename H3Fallback<C>::X;
            if (__syncthreads_or(ovf)) {
                if ((tid >> 8) == 0)
                    nn_h3_fallback<X, X::GRP0>(pv.leaf_state, span, xblob, blocks, pv.policy, pv.value, lds);
                else
                    nn_h3_fallback<X, X::GRP1>(pv.leaf_state, span, xblob, blocks, pv.policy, pv.value, lds);
                if (tid == 0) atomicAdd(fallback, 1ull);
            }
        }
        __syncthreads();  // the evaluation rows written; the LDS is the tree's again
        if (walker) par_backup(tg, rg, pol, val, m, sp);
        done += m;
        ++rounds;
        __syncthreads();  // round_m is read before the next round writes it
    }
    if (tid == 0) {
        pv.lb_stats[(size_t)g * 3 + 0] = rounds;
        pv.lb_stats[(size_t)g * 3 + 1] = done;
        pv.lb_stats[(size_t)g * 3 + 2] = discarded;
        if (deadline) sims_run[g] = done;
    }
}

hipError_t launch_search_par(const TreeView& t, const oaz_state* roots, SearchParams p, int sims, int leaf_batch,
                             const NNView* w, const ParBufs& b, const uint64_t* deadline, uint32_t* sims_run,
                             hipStream_t st) {
    if (deadline && !sims_run) return hipErrorInvalidValue;
    if (leaf_batch < 1 || leaf_batch > nn::kSB || !b.path || !b.depth || !b.leaf || !b.leaf_state || !b.policy ||
        !b.value || !b.lb_stats)
        return hipErrorInvalidValue;
    if (t.G == 0 || sims <= 0) return hipSuccess;
    if (w && (!w->fallback || !w->blob_x6 || w->precision != OAZ_FP32_SPLIT16)) return hipErrorInvalidValue;
    const ParView pv{b.path, b.depth, b.leaf, b.leaf_state, b.policy, b.value, b.lb_stats, (uint32_t)leaf_batch};
    hipLaunchKernelGGL(k_search_par, dim3(t.G), dim3(kLatThreads), 0, st, t, pv, roots, p, sims, w ? 0 : 1,
                       w ? w->blob : nullptr, w ? w->blocks : 0, w ? w->blob_x6 : nullptr, w ? w->fallback : nullptr,
                       deadline, sims_run);
    return hipGetLastError();
}

}  // namespace oaz
