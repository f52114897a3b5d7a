// oaz_pack.h — canonical network weights -> the packed device image (oaz_nn_layout.h). Pure host
// code: no HIP, no engine.
#pragma once

#include <stddef.h>

#include <vector>

enum { OAZ_PACK_OK = 0, OAZ_PACK_BAD_ARG = 1, OAZ_PACK_RAW_SIZE = 2 };

// Folds BN into the convs and packs raw[raw_floats] (the canonical blob of oaz_weights_layout.h) for
// `precision` into out, resized to nn_device_floats(blocks, precision). Returns OAZ_PACK_OK or a code above.
int oaz_pack_weights(const float* raw, size_t raw_floats, int blocks, int precision, std::vector<float>& out);
