// oaz_playout_cap.hip — playout cap randomization in self-play (oaz_selfplay_set_playout_cap).
// Part of oaz_gpu.hip's translation unit, after oaz_kernels.hip: the capped ply is selfplay_move_body with kCap, and
// its records go out through k_samples_scan / k_samples_emit as every other ply's.
//
// A capped ply is searched in two phases (run_capped, oaz_engine.cpp): every active game runs the first fast_sims
// playouts, only the games whose ply is a full one run the rest. The tree, compaction, network and noise kernels take
// a per-game mask in the form of SlotView::active and leave a game whose byte is not 1 alone, so the two phases are
// two masks; this file makes them, and plays the ply.
namespace oaz {

// One thread per slot: full = the rule (playout_cap_full, oaz_device.h) for the slot's game id and ply, whatever the
// slot's state; fast / fullm = the slot is playing (active == 1; 0 = finished, > 1 = still waiting for its staggered
// start) and its ply is a fast / a full one. 20 bytes read and 3 written per slot and one Philox block: nothing here
// is worth more than coalesced accesses.
__global__ void __launch_bounds__(kBlock) k_playout_cap_masks(SlotView sv, CapView cv) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= sv.G) return;
    const bool full = playout_cap_full(sv.seed, sv.game_id[g], sv.ply[g], cv.P);
    const bool on = sv.active[g] == 1;
    cv.full[g] = full ? 1 : 0;
    cv.fast[g] = on && !full ? 1 : 0;
    cv.fullm[g] = on && full ? 1 : 0;
}

// temp_plies = 0: no ply draws its move (ply < 0 never holds) and cnt is never read.
__global__ void __launch_bounds__(kBlock) k_selfplay_move_cap(TreeView t, SlotView sv, CapView cv, uint32_t temp_plies,
                                                              unsigned long long* cnt) {
    selfplay_move_body<true, true>(t, sv, temp_plies, cnt, cv);
}

hipError_t launch_playout_cap_masks(const SlotView& s, const CapView& c, hipStream_t st) {
    hipLaunchKernelGGL(k_playout_cap_masks, dim3(thread_grid(s.G, kBlock)), dim3(kBlock), 0, st, s, c);
    return hipGetLastError();
}

hipError_t launch_selfplay_move_cap(const TreeView& t, const SlotView& s, const CapView& c, uint32_t temp_plies,
                                    uint64_t* temp_counters, hipStream_t st) {
    hipLaunchKernelGGL(k_selfplay_move_cap, dim3(wave_grid(t.G)), dim3(kBlock), 0, st, t, s, c, temp_plies,
                       reinterpret_cast<unsigned long long*>(temp_counters));
    hipLaunchKernelGGL(k_samples_scan, dim3(1), dim3(kScanThreads), 0, st, s);
    hipLaunchKernelGGL(k_samples_emit, dim3(wave_grid(t.G)), dim3(kBlock), 0, st, t, s);
    return hipGetLastError();
}

}  // namespace oaz
