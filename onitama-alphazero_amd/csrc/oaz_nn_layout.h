// oaz_nn_layout.h — the one description of the packed, BN-folded NN weight blob: oaz_pack.cpp writes
// it, the kernels in oaz_nn.hip / oaz_search_lat.hip read it, tests/test_pack.py checks it on the CPU.
// Plain C++17 and HIP (no hip_runtime.h). All offsets and lengths are in floats; 16-bit fragments are
// stored two to a float.
//
// Packed blob of one precision, `blocks` residual blocks:
//   first layer (every precision, the exact-fp32 encoding):
//     [L1 B: 9 taps x 4 N-tiles x 64 lanes][L1 bias 64][L1 table T: 25 squares x 17 x 64]
//   2 * blocks convs 64->64, each [B fragments][tail]:
//     OAZ_FP32          [9 taps][4 k-groups][4 N-tiles][64 lanes] f32x4            | bias[64]
//     OAZ_BF16          [9 taps][2 K-halves][4 N-tiles][64 lanes] bf16x8           | bias[64]
//     OAZ_FP32_SPLIT    [9 taps][2 K-halves][3 pieces][4 N-tiles][64 lanes] bf16x8 | bias[64]
//     OAZ_FP32_SPLIT16  [9 taps][2 K-halves][2 pieces][4 N-tiles][64 lanes] f16x8  | bias[64] 1/s[64]
//       (the weights of output channel co scaled by s_co = 2^k)
//   heads (every precision; offsets below are relative to heads()):
//     value:  wv[64] bv pad[3] l1w[25][64] (transposed) l1b[64] l2w[64] l2b pad[3]
//     policy: wp[2][64] bp[2] pad[2] plw[50 in][50 out] (transposed) plb[50] pad[2]
//   head 1x1 convs as B fragments, columns 0 = value conv, 1 / 2 = policy planes, 3..15 zero (not OAZ_FP32):
//     OAZ_BF16          [2 K-halves][64 lanes] bf16x8
//     OAZ_FP32_SPLIT    [2 K-halves][3 pieces][64 lanes] bf16x8
//     OAZ_FP32_SPLIT16  [2 K-halves][2 pieces][64 lanes] f16x8 of the column-scaled weights | 1/s[3] pad[1]
//   first layer on fp16 MFMA (OAZ_FP32_SPLIT16 and OAZ_BF16), scaled by s_co = 2^k per output channel:
//     [K block 0: 2 pieces x 4 N-tiles x 64 lanes f16x8][K block 1 of each of the 25 squares, same shape] | 1/s[64]
// The device image of OAZ_FP32_SPLIT16 is its blob followed by the OAZ_FP32_SPLIT blob of the same
// weights (fp16-range tiles are recomputed with it): nn_device_floats().
#pragma once

#include <stddef.h>

#include <string>
#include <vector>

#include "../../include/onitama_az.h"

#ifndef OAZ_HD  // (oaz_device.h defines the same macro)
#if defined(__HIP__)
#define OAZ_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define OAZ_HD inline
#endif
#endif

namespace oaz {
namespace nnl {

constexpr size_t kCh = 64;

// ---- first layer, exact-fp32 encoding (from the blob's start) ----
constexpr size_t kL1B = 0;  // bitboard planes' B fragments
constexpr size_t kL1BLen = 9 * 4 * 64;
constexpr size_t kL1Bias = kL1B + kL1BLen;
constexpr size_t kL1Table = kL1Bias + kCh;  // T[square][c][co]: the 16 card planes and the colour plane
constexpr size_t kL1TableLen = 25 * 17 * kCh;
constexpr size_t kConvs = kL1Table + kL1TableLen;  // the first 64->64 conv

// ---- one 64->64 conv: conv_w() floats of B fragments, then the tail ----
OAZ_HD constexpr size_t pieces(int prec) {  // 16-bit terms per weight (0: fp32 fragments)
    return prec == OAZ_BF16 ? 1 : prec == OAZ_FP32_SPLIT ? 3 : prec == OAZ_FP32_SPLIT16 ? 2 : 0;
}
OAZ_HD constexpr size_t conv_w(int prec) {
    return prec == OAZ_FP32 ? 9 * 4 * 4 * 64 * 4 : 9 * 2 * pieces(prec) * 4 * 64 * 4;
}
constexpr size_t kConvBias = 0;   // within the tail
constexpr size_t kConvInv = kCh;  // OAZ_FP32_SPLIT16: the inverse scales 1/s[64]
OAZ_HD constexpr size_t conv_tail(int prec) { return prec == OAZ_FP32_SPLIT16 ? 2 * kCh : kCh; }
OAZ_HD constexpr size_t conv_stride(int prec) { return conv_w(prec) + conv_tail(prec); }

// ---- heads: offset in the blob, then fields relative to it ----
OAZ_HD constexpr size_t heads(int prec, int blocks) { return kConvs + (size_t)blocks * 2 * conv_stride(prec); }
constexpr size_t kWv = 0;           // value 1x1 conv (BN folded) [64]
constexpr size_t kBv = kWv + kCh;   // its bias, pad[3]
constexpr size_t kL1w = kBv + 4;    // vh_linear1.weight transposed [25][64]
constexpr size_t kL1b = kL1w + 25 * kCh;
constexpr size_t kL2w = kL1b + kCh;  // vh_linear2.weight [64]
constexpr size_t kL2b = kL2w + kCh;  // its bias, pad[3]
constexpr size_t kWp = kL2b + 4;     // policy 1x1 conv (BN folded) [2][64]
constexpr size_t kBp = kWp + 2 * kCh;  // its biases [2], pad[2]
constexpr size_t kPlw = kBp + 4;       // ph_linear2.weight transposed [50 in][50 out]
constexpr size_t kPlb = kPlw + 50 * 50;  // its bias [50], pad[2]
constexpr size_t kHeadB = kPlb + 52;     // the head 1x1 convs' B fragments
OAZ_HD constexpr size_t head_b(int prec) { return 2 * pieces(prec) * 64 * 4; }
OAZ_HD constexpr size_t head_inv(int prec) { return kHeadB + head_b(prec); }  // OAZ_FP32_SPLIT16: 1/s[3], pad[1]
OAZ_HD constexpr size_t heads_len(int prec) { return head_inv(prec) + (prec == OAZ_FP32_SPLIT16 ? 4 : 0); }

// ---- first layer on fp16 MFMA: offset in the blob, then fields relative to it ----
OAZ_HD constexpr bool has_l1c(int prec) { return prec == OAZ_FP32_SPLIT16 || prec == OAZ_BF16; }
OAZ_HD constexpr size_t l1c(int prec, int blocks) { return heads(prec, blocks) + heads_len(prec); }
constexpr size_t kL1Frag = 2 * 4 * 64 * 4;  // one K block: 2 pieces x 4 N-tiles x 64 lanes x f16x8
constexpr size_t kL1cK1 = kL1Frag;          // K block 1 of square 0 (K block 0 at 0)
constexpr size_t kL1cInv = 26 * kL1Frag;    // 1/s[64]
constexpr size_t kL1cLen = kL1cInv + kCh;

OAZ_HD constexpr size_t total(int prec, int blocks) {
    return l1c(prec, blocks) + (has_l1c(prec) ? kL1cLen : 0);
}

// ---- the kernels' forms: per-precision constants (P a compile-time precision) ----
template <int P> constexpr size_t kConvW = conv_w(P);
template <int P> constexpr size_t kConvTail = conv_tail(P);
template <int P> constexpr size_t kConvStride = conv_stride(P);
template <int P> constexpr size_t kHeadBLen = head_b(P);
template <int P> constexpr size_t kHeadInv = head_inv(P);
template <int P> constexpr size_t kHeadsLen = heads_len(P);

}  // namespace nnl

// kConvs, heads() and l1c() as pointers into `blob` for the kernels. Macros that walk the regions in order: the
// address arithmetic is then compiled in the kernel's own body in the shape (blob + kL1Bias) + ... + run-time part
// + constant, sharing its first terms with the kernel's other first-layer addresses. (One merged constant, or a
// helper function, which is simplified on its own before it is inlined, gives different if equivalent code.)
#define OAZ_NN_CONVS_AT(blob) ((blob) + oaz::nnl::kL1Bias + oaz::nnl::kCh + oaz::nnl::kL1TableLen)
#define OAZ_NN_HEADS_AT(blob, P, blocks) (OAZ_NN_CONVS_AT(blob) + (size_t)(blocks) * 2 * oaz::nnl::kConvStride<P>)
#define OAZ_NN_L1C_AT(blob, P, blocks) (OAZ_NN_HEADS_AT(blob, P, blocks) + oaz::nnl::kHeadsLen<P>)
static_assert(oaz::nnl::kL1Bias + oaz::nnl::kCh + oaz::nnl::kL1TableLen == oaz::nnl::kConvs, "OAZ_NN_CONVS_AT");

// Floats of the packed blob of one precision (oaz_nn_device_bytes / 4).
inline size_t nn_packed_floats(int blocks, int precision) { return nnl::total(precision, blocks); }
// Floats of an engine's device image (OAZ_FP32_SPLIT16 carries the OAZ_FP32_SPLIT blob for its fallback).
inline size_t nn_device_floats(int blocks, int precision) {
    return nnl::total(precision, blocks) + (precision == OAZ_FP32_SPLIT16 ? nnl::total(OAZ_FP32_SPLIT, blocks) : 0);
}

// The device image as an ordered table of named sections that tile [0, nn_device_floats) (a field's
// padding belongs to its section; the appended OAZ_FP32_SPLIT blob's names carry the prefix "x6.").
struct NNSection {
    std::string name;
    size_t off, len;
};
inline std::vector<NNSection> nn_sections(int blocks, int precision) {
    using namespace nnl;
    std::vector<NNSection> s;
    auto blob = [&](int prec, size_t base, const std::string& pre) {
        auto add = [&](const std::string& name, size_t off, size_t end) { s.push_back({pre + name, base + off, end - off}); };
        add("l1.b", kL1B, kL1Bias);
        add("l1.bias", kL1Bias, kL1Table);
        add("l1.table", kL1Table, kConvs);
        for (int c = 0; c < 2 * blocks; ++c) {
            const size_t o = kConvs + (size_t)c * conv_stride(prec), t = o + conv_w(prec);
            const std::string n = "conv" + std::to_string(c);
            add(n + ".w", o, t);
            add(n + ".bias", t + kConvBias, t + kCh);
            if (prec == OAZ_FP32_SPLIT16) add(n + ".inv", t + kConvInv, t + conv_tail(prec));
        }
        const size_t h = heads(prec, blocks);
        const size_t f[] = {kWv, kBv, kL1w, kL1b, kL2w, kL2b, kWp, kBp, kPlw, kPlb, kHeadB};
        const char* const fn[] = {"value.wv",  "value.bv",  "value.l1w",  "value.l1b",  "value.l2w",
                                  "value.l2b", "policy.wp", "policy.bp", "policy.plw", "policy.plb"};
        for (int k = 0; k < 10; ++k) add(fn[k], h + f[k], h + f[k + 1]);
        if (prec != OAZ_FP32) add("head.b", h + kHeadB, h + head_inv(prec));
        if (prec == OAZ_FP32_SPLIT16) add("head.inv", h + head_inv(prec), h + heads_len(prec));
        if (has_l1c(prec)) {
            const size_t l = l1c(prec, blocks);
            add("l1c.k0", l, l + kL1cK1);
            add("l1c.k1", l + kL1cK1, l + kL1cInv);
            add("l1c.inv", l + kL1cInv, l + kL1cLen);
        }
    };
    blob(precision, 0, "");
    if (precision == OAZ_FP32_SPLIT16) blob(OAZ_FP32_SPLIT, total(precision, blocks), "x6.");
    return s;
}

}  // namespace oaz
