// oaz_tree_rebase.h — re-rooting a search tree at a child of its root (tree reuse), stated once for the host
// (oaz_tree_rebase_host, oaz_tree_rebase.cpp) and the device (tree_rebase, oaz_tree_reuse.hip).
//
// The fact it rests on (DESIGN.md "Tree reuse"): node indices are allocation order and the playouts that pass
// through a root child c see only c's subtree, so that subtree, taken out with its node order kept, IS the tree
// of a fresh search from c's position with N_c playouts, node for node, once the new root carries what a fresh
// root does (P = 1, mv = 0; mcts_arena.rs:57).
//
//   which nodes   c, and with every member that is expanded its children block [first, first + nch). A block
//                 always lies above its parent (it was allocated when the parent was expanded);
//   which order   ascending old index (a stable compaction): a member's new index is the number of members
//                 below it, so a new index is never greater than the old one;
//   which remap   an expanded member's `first` becomes the number of members below the old `first` (the new
//                 index of its first child, or with no child the node count of the fresh search at that
//                 expansion); every other field is kept, pad stays 0.
#pragma once

#include <stdint.h>

#include "../../include/onitama_az.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OAZ_RB_HD __host__ __device__ __forceinline__
#else
#define OAZ_RB_HD inline
#endif

namespace oaz {
namespace rebase {

constexpr uint32_t kExpanded = 1, kTerminal = 2;  // oaz_node.flags

// Which nodes: the children a member brings with it, [first, first + block_len).
OAZ_RB_HD uint32_t block_len(uint32_t flags, uint32_t nch) { return (flags & kExpanded) ? nch : 0u; }
// Which remap: `first` is rewritten for expanded nodes only (an unexpanded node's is not defined).
OAZ_RB_HD bool remaps_first(uint32_t flags) { return (flags & kExpanded) != 0; }
// The new root is a fresh search's root (mcts_arena.rs:57).
constexpr double kRootP = 1.0;
constexpr uint32_t kRootMv = 0;

// The keep rule, the same everywhere: the tree of root child c is kept when the root is expanded, c is expanded
// and not terminal-flagged, the move to c does not win, and c's visits plus a search's playouts (sims_cap, the
// creation budget) fit the trees' capacity R in root visits; otherwise the next search starts from a fresh tree.
OAZ_RB_HD bool keeps(uint32_t root_flags, uint32_t child_flags, uint32_t child_N, bool move_wins, int32_t sims_cap,
                     int32_t R) {
    return (root_flags & kExpanded) && (child_flags & kExpanded) && !(child_flags & kTerminal) && !move_wins &&
           (uint64_t)child_N + (uint64_t)sims_cap <= (uint64_t)R;
}

// The sequential statement. in[0, n): a tree in allocation order; child: which of the root's children (0 ..
// nch - 1) becomes the root. out[0, *n_out) receives the re-rooted tree (out must not overlap in). Returns 0,
// OAZ_ERR_ARG (no such child, an unvisited child, a block outside the tree) or OAZ_ERR_CAPACITY (cap too
// small); on an error nothing is written. `rank` is scratch of n + 1 entries.
inline int host(const oaz_node* in, int n, int child, oaz_node* out, int cap, int* n_out, uint32_t* rank) {
    if (!in || n < 1 || child < 0 || !rank) return OAZ_ERR_ARG;
    const oaz_node& root = in[0];
    if (child >= (int)block_len(root.flags, root.nch)) return OAZ_ERR_ARG;
    const uint32_t c = root.first + (uint32_t)child;
    if (c < 1 || c >= (uint32_t)n || in[c].N == 0) return OAZ_ERR_ARG;
    // rank[i] = members below i, the top bit = i is a member; one ascending pass, as blocks lie above their parents
    constexpr uint32_t kMember = 0x80000000u;
    for (int i = 0; i <= n; ++i) rank[i] = 0;
    rank[c] = kMember;
    uint32_t count = 0;
    for (uint32_t i = c; i < (uint32_t)n; ++i) {
        const bool member = (rank[i] & kMember) != 0;
        rank[i] = (rank[i] & kMember) | count;
        if (!member) continue;
        ++count;
        const uint32_t len = block_len(in[i].flags, in[i].nch);
        if (len && (in[i].first <= i || (uint64_t)in[i].first + len > (uint64_t)n)) return OAZ_ERR_ARG;
        for (uint32_t k = 0; k < len; ++k) rank[in[i].first + k] |= kMember;
    }
    rank[n] = count;
    if (!out || (int64_t)count > (int64_t)cap) return OAZ_ERR_CAPACITY;
    for (uint32_t i = c; i < (uint32_t)n; ++i) {
        if (!(rank[i] & kMember)) continue;
        oaz_node m = in[i];
        if (remaps_first(m.flags)) m.first = rank[m.first < (uint32_t)n ? m.first : (uint32_t)n] & ~kMember;
        m.pad = 0;
        out[rank[i] & ~kMember] = m;
    }
    out[0].P = kRootP;
    out[0].mv = (uint16_t)kRootMv;
    if (n_out) *n_out = (int)count;
    return 0;
}

}  // namespace rebase
}  // namespace oaz
