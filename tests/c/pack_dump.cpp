// pack_dump — packs canonical float32 weights on the CPU (csrc/oaz_pack.cpp, no library, no GPU):
//   pack_dump RAW.f32 BLOCKS PRECISION OUT.bin
// writes the device image to OUT.bin and prints
//   packed_floats N / device_floats N / section NAME OFFSET LENGTH ...   (oaz_nn_layout.h)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../onitama-alphazero_amd/csrc/oaz_nn_layout.h"
#include "../../onitama-alphazero_amd/csrc/oaz_pack.h"

int main(int argc, char** argv) {
    if (argc != 5) return fprintf(stderr, "usage: pack_dump RAW.f32 BLOCKS PRECISION OUT.bin\n"), 2;
    const int blocks = atoi(argv[2]), precision = atoi(argv[3]);
    FILE* in = fopen(argv[1], "rb");
    if (!in) return perror(argv[1]), 2;
    std::vector<float> raw;
    float buf[4096];
    for (size_t n; (n = fread(buf, sizeof(float), 4096, in)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(in);
    std::vector<float> blob;
    if (int rc = oaz_pack_weights(raw.data(), raw.size(), blocks, precision, blob))
        return fprintf(stderr, "oaz_pack_weights: code %d (%zu raw floats)\n", rc, raw.size()), 1;
    FILE* out = fopen(argv[4], "wb");
    if (!out || fwrite(blob.data(), sizeof(float), blob.size(), out) != blob.size() || fclose(out) != 0)
        return perror(argv[4]), 2;
    printf("packed_floats %zu\n", oaz::nn_packed_floats(blocks, precision));
    printf("device_floats %zu\n", blob.size());
    for (const oaz::NNSection& s : oaz::nn_sections(blocks, precision))
        printf("section %s %zu %zu\n", s.name.c_str(), s.off, s.len);
    return 0;
}
