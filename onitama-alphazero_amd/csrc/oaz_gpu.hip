// oaz_gpu.hip — one translation unit for the rules / search kernels (oaz_kernels.hip), the network
// kernels (oaz_nn.hip), the one-launch small-batch search (oaz_search_lat.hip), which inlines the
// device bodies of both (tree walk + network in one workgroup), the leaf-parallel search (oaz_search_par.hip),
// which does the same with a tile of leaves per root, tree reuse (oaz_tree_reuse.hip), which uses the tree
// kernels' device helpers, and playout cap randomization (oaz_playout_cap.hip), whose ply kernel is the self-play
// ply's body.
#include "oaz_kernels.hip"
#include "oaz_nn.hip"
#include "oaz_search_lat.hip"
#include "oaz_search_par.hip"
#include "oaz_tree_reuse.hip"
#include "oaz_playout_cap.hip"
