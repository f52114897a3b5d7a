// oaz_tree_rebase.cpp — oaz_tree_rebase_host: the host restatement of the device's tree re-rooting
// (oaz_tree_rebase.h states the compaction for both). Host only, plain C++: nothing here needs HIP.
#include <vector>

#include "../../include/onitama_az.h"
#include "oaz_tree_rebase.h"

#ifdef OAZ_REBASE_STANDALONE  // this file alone (a sanitizer build for a C program): no oaz_last_error to write
static int oaz_set_err(int code, const char*, ...) { return code; }
#else
int oaz_set_err(int code, const char* fmt, ...);  // oaz_host.h (which needs the HIP headers)
#endif

extern "C" int oaz_tree_rebase_host(const oaz_node* in, int n, int child, oaz_node* out, int cap, int* n_out) {
    if (!in || n < 1) return oaz_set_err(OAZ_ERR_ARG, "tree_rebase_host: no tree");
    std::vector<uint32_t> rank((size_t)n + 1);
    const int rc = oaz::rebase::host(in, n, child, out, cap, n_out, rank.data());
    if (rc == OAZ_ERR_CAPACITY) return oaz_set_err(rc, "tree_rebase_host: the subtree does not fit cap=%d nodes", cap);
    if (rc) return oaz_set_err(rc, "tree_rebase_host: child %d of a %d-node tree is no visited child of the root", child, n);
    return 0;
}
