// oaz_pack.h — canonical network weights -> the packed device image (oaz_nn_layout.h). Pure host
// code: no HIP, no engine.
#pragma once

#include <stddef.h>

#include <vector>

enum { OAZ_PACK_OK = 0, OAZ_PACK_BAD_ARG = 1, OAZ_PACK_RAW_SIZE = 2 };

// Floats of the canonical weights of a `blocks`-block network (64 channels, 21 input planes).
size_t oaz_pack_raw_floats(int blocks);

// Folds BN into the convs and packs raw[raw_floats] (canonical order, DESIGN.md "Weights") for
// `precision` into out, resized to nn_device_floats(blocks, precision). Returns OAZ_PACK_OK or a code above.
int oaz_pack_weights(const float* raw, size_t raw_floats, int blocks, int precision, std::vector<float>& out);
