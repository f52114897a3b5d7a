// oaz_search_par.hip — leaf-parallel search with virtual loss (oaz_config.leaf_batch = L, 1 <= L <= 16;
// DESIGN.md "Leaf-parallel search"): the whole search of a few roots in ONE launch, one workgroup per root as
// k_search_lat, but a network pass evaluates up to L leaves of the SAME tree as one 16-position tile (nn_h3_tile,
// oaz_nn.hip).
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
// and the back up sequentially in j; all eight waves evaluate the tile. The walk is select_wide_body
// (oaz_kernels.hip) on the effective statistics, the tile evaluation nn_h3_tile (oaz_nn.hip).
//
// The tree, the paths and the leaf records stay in global memory (L2): the tile body and its fp16-range
// recompute use the kernel's whole LDS (H3Fallback::kLds, 157.7 KB of 160), which leaves no room for an LDS
// copy of the top of the tree beside them.
//
// Q7 search_time: thread 0 reads the device clock before every round after the first; a search stops only at a
// round boundary, sims_run[g] = done.
namespace oaz {

__device__ __forceinline__ void par_fence() {  // the walker wave's own stores, visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The collect phase of one round on the walker wave (all 64 lanes): up to `want` walks of select_wide_body on
// the effective statistics. t is the root's own view (G = 1; path / depth / leaf / leaf_state: leaf 0's records,
// leaf j's follow at j * pathcap, j, j, j). Returns the leaves collected (uniform); *disc = 1 when a discarded
// walk closed the round.
__device__ __noinline__ uint32_t par_collect(const TreeView& t, const oaz_state* root, const SearchParams& prm,
                                             uint32_t want, uint32_t* disc) {
    const int l = (int)(threadIdx.x & 63);
    oaz_node* T = t.nodes;
    uint32_t m = 0;
    *disc = 0;
    for (uint32_t j = 0; j < want; ++j) {
        uint32_t* path = t.path + (size_t)j * t.pathcap;
        WideLeaf<true> w;
        select_wide_body<NodesGlobalRegs, true, 0>(w, t, T, path, root, prm, NodesGlobalRegs{});
        if (!(node_flags(w.nd.misc) & 3) && w.nd.v > 0) {  // this leaf is already in flight: the round closes here
            *disc = 1;
            par_fence();  // (a terminal flag the walk set)
            break;
        }
        if (l == 0) {
            const bool need = leaf_needs_eval(w.nd.misc, w.s);
            store_state(t.leaf_state + j, w.s);
            t.leaf[j] = w.node;
            t.depth[j] = w.depth;
            t.stats[GS_SIMS] += 1;  // one writer: this lane
            t.stats[GS_DEPTH] += w.depth;
            t.stats[GS_EVALS] += need;
            if (w.stuck) t.stats[GS_STUCK] += 1;
        }
        par_fence();  // the path, written by lane 0
        const uint32_t plen = w.depth < t.pathcap ? w.depth : t.pathcap - 1;
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

__global__ void __launch_bounds__(kLatThreads) k_search_par(TreeView t, ParBufs pv, const oaz_state* __restrict__ roots,
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
            nn_h3_tile<C>(pv.leaf_state, span, blob, blocks, xblob, fallback, pv.policy, pv.value, lds, opaque);
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

hipError_t launch_search_par(const TreeView& t, const oaz_state* roots, SearchParams p, int sims, const NNView* w,
                             const ParBufs& b, const uint64_t* deadline, uint32_t* sims_run, hipStream_t st) {
    if (hipError_t bad = search_args_check(deadline, sims_run, w)) return bad;
    if (b.L < 1 || b.L > (uint32_t)nn::kSB || !b.path || !b.depth || !b.leaf || !b.leaf_state || !b.policy ||
        !b.value || !b.lb_stats)
        return hipErrorInvalidValue;
    if (t.G == 0 || sims <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_search_par, dim3(t.G), dim3(kLatThreads), 0, st, t, b, roots, p, sims, w ? 0 : 1,
                       w ? w->blob : nullptr, w ? w->blocks : 0, w ? w->blob_x6 : nullptr, w ? w->fallback : nullptr,
                       deadline, sims_run);
    return hipGetLastError();
}

}  // namespace oaz
