// weights_layout_dump — prints the canonical weight blob's layout (csrc/oaz_weights_layout.h alone:
// no library, no GPU):
//   weights_layout_dump BLOCKS [CHANNELS IN_PLANES]
// prints
//   tensor NAME SHAPE(d0,d1,...) OFFSET NUMEL RUNNING_STAT    per tensor, creation order
//   total N
//   bn_segment OFFSET LENGTH                                  running statistics, pack order
//   sgd_run VALUE OFFSET LENGTH                               maximal runs of the SGD mask
#include <stdio.h>
#include <stdlib.h>

#include "../../onitama-alphazero_amd/csrc/oaz_weights_layout.h"

int main(int argc, char** argv) {
    if (argc != 2 && argc != 4) return fprintf(stderr, "usage: weights_layout_dump BLOCKS [CHANNELS IN_PLANES]\n"), 2;
    using namespace oaz::wl;
    const Layout L = argc == 4 ? layout(atoi(argv[1]), (size_t)atoi(argv[2]), (size_t)atoi(argv[3])) : layout(atoi(argv[1]));
    for (const Tensor& t : L.tensors) {
        printf("tensor %s ", t.name.c_str());
        for (size_t d = 0; d < t.shape.size(); ++d) printf(d ? ",%zu" : "%zu", t.shape[d]);
        printf(" %zu %zu %d\n", t.offset, t.numel, (int)t.running_stat);
    }
    printf("total %zu\n", L.total);
    for (const Run& r : running_stat_runs(L)) printf("bn_segment %zu %zu\n", r.offset, r.len);
    const std::vector<uint8_t> mask = sgd_mask(L);
    for (size_t i = 0, j; i < mask.size(); i = j) {
        for (j = i; j < mask.size() && mask[j] == mask[i]; ++j) {}
        printf("sgd_run %d %zu %zu\n", (int)mask[i], i, j - i);
    }
    return 0;
}
