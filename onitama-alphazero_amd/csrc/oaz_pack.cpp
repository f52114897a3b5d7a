// oaz_pack.cpp — weights: canonical (tch VarStore order) -> BN-folded -> MFMA-packed, written at the
// offsets of oaz_nn_layout.h into a zero-initialised image (so every pad is zero). The canonical
// blob is read at the offsets of oaz_weights_layout.h.
#include "oaz_pack.h"

#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "oaz_nn_layout.h"
#include "oaz_weights_layout.h"

using namespace oaz;

namespace {

struct FoldedConv {
    std::vector<float> w;  // [cout][cin][taps]
    std::vector<float> b;  // [cout]
};

FoldedConv fold(const float* raw, const wl::ConvBn& c) {
    FoldedConv f;
    const float *w = raw + c.w, *b = raw + c.b, *g = raw + c.gamma, *beta = raw + c.beta, *mean = raw + c.mean,
                *var = raw + c.var;
    const size_t per = c.cin * c.k * c.k;  // weights per output channel
    f.w.resize(c.cout * per);
    f.b.resize(c.cout);
    for (size_t o = 0; o < c.cout; ++o) {
        const double s = (double)g[o] / sqrt((double)var[o] + 1e-5);  // BN eval, eps 1e-5
        for (size_t k = 0; k < per; ++k) f.w[o * per + k] = (float)((double)w[o * per + k] * s);
        f.b[o] = (float)(((double)b[o] - (double)mean[o]) * s + (double)beta[o]);
    }
    return f;
}

// ---- element conversions: one fp32 weight -> pieces(precision) 16-bit terms ----------------------
uint16_t f32_to_bf16(float f) {  // round to nearest even
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// fp32 split (OAZ_FP32_SPLIT): w = hi + mid + lo exactly, each term the top 16 bits of an fp32
// (8 significant bits: bf16). hi = trunc(w), mid = trunc(w - hi), lo = w - hi - mid (both
// subtractions exact, lo has <= 8 significant bits). Same split as split3() in oaz_nn.hip.
void split3_host(float w, uint16_t out[3]) {
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto from = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    const uint32_t h = bits(w) & 0xffff0000u;
    const float r = w - from(h);
    const uint32_t m = bits(r) & 0xffff0000u;
    const float l = r - from(m);
    out[0] = (uint16_t)(h >> 16);
    out[1] = (uint16_t)(m >> 16);
    out[2] = (uint16_t)(bits(l) >> 16);
}

// fp16 split (OAZ_FP32_SPLIT16): hi = fp16(x) (round to nearest even), lo = fp16(x - hi); the same
// split as epilogue_h3_pack in oaz_nn.hip. Weights are first scaled by s = 2^k per output channel so
// that max |w s| lies in [2^14, 2^15): the top of fp16's range (products with activations < 65504
// stay far inside fp32), which keeps hi normal for weights down to 2^-28 of the channel's largest and
// bounds each weight's representation error by 2^-25 / s = 2^-39 max|w| (a channel with one huge
// weight no longer pushes its ordinary weights into fp16 subnormals). 1/s is stored for the epilogue.
void split16_host(float x, uint16_t out[2]) {
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    memcpy(&out[0], &h, 2);
    memcpy(&out[1], &l, 2);
}
float pow2_scale(const float* w, size_t n, size_t stride, float* inv) {
    float mx = 0.0f;
    for (size_t k = 0; k < n; ++k) mx = fmaxf(mx, fabsf(w[k * stride]));
    if (!(mx > 0.0f) || !std::isfinite(mx)) {
        *inv = 1.0f;
        return 1.0f;
    }
    int e = 0;
    (void)frexpf(mx, &e);  // mx = f 2^e, f in [0.5, 1)
    if (e < -100) e = -100;  // keep s and 1/s normal floats
    *inv = ldexpf(1.0f, e - 15);
    return ldexpf(1.0f, 15 - e);
}

void split(int prec, float w, uint16_t out[3]) {
    if (prec == OAZ_BF16) out[0] = f32_to_bf16(w);
    else if (prec == OAZ_FP32_SPLIT) split3_host(w, out);
    else split16_host(w, out);
}

// ---- 16x16x32 MFMA operand fragments -----------------------------------------------------------
// Write cursor over a region of the image, in 16-bit elements.
struct Cursor16 {
    float* base;
    size_t n = 0;
    void put(uint16_t v) { memcpy(reinterpret_cast<char*>(base) + 2 * n++, &v, 2); }
};

// [piece][tile][64 lanes] x8: lane l's element e is piece `pc` of w(tile, l, e).
template <class W>
void put_frags(Cursor16& c, int prec, int tiles, W&& w) {
    for (size_t pc = 0; pc < nnl::pieces(prec); ++pc)
        for (int nt = 0; nt < tiles; ++nt)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    uint16_t s[3];
                    split(prec, w(nt, l, e), s);
                    c.put(s[pc]);
                }
}

// A 64->64 conv for the 16x16x32 layouts: [tap][K-half m][piece][N-tile][lane] x8, lane l supplying
// B[k = 8(l>>4) + e][col l&15] = piece of W[co = 16nt + (l&15)][ci = 32m + 8(l>>4) + e][tap], for
// OAZ_FP32_SPLIT16 of s_co W with s_co = 2^k; then the tail: bias[64] (and 1/s[64]).
void pack_conv64_x32(const FoldedConv& f, int prec, float* out) {
    const bool scaled = prec == OAZ_FP32_SPLIT16;
    float sc[64], inv[64];
    if (scaled)
        for (int co = 0; co < 64; ++co) sc[co] = pow2_scale(&f.w[(size_t)co * 64 * 9], 64 * 9, 1, &inv[co]);
    Cursor16 c{out};
    for (int t = 0; t < 9; ++t)
        for (int m = 0; m < 2; ++m)
            put_frags(c, prec, 4, [&](int nt, int l, int e) {
                const int co = nt * 16 + (l & 15), ci = 32 * m + 8 * (l >> 4) + e;
                const float w = f.w[((size_t)co * 64 + ci) * 9 + t];
                return scaled ? w * sc[co] : w;  // exact scaling
            });
    assert(c.n == 2 * nnl::conv_w(prec));
    float* tail = out + nnl::conv_w(prec);
    memcpy(tail + nnl::kConvBias, f.b.data(), 64 * sizeof(float));
    if (scaled) memcpy(tail + nnl::kConvInv, inv, 64 * sizeof(float));
}

// B fragments of v_mfma_f32_16x16x4f32 for a 64->64 conv (OAZ_FP32): lane l supplies B[k=l>>4][col=l&15];
// k-group g of tap t covers channels ci = 16g + 4(l>>4) + q, q = 0..3; N-tile nt = 16 columns. Then bias[64].
void pack_conv64_f32(const FoldedConv& f, float* out) {
    float* o = out;
    for (int t = 0; t < 9; ++t)
        for (int g = 0; g < 4; ++g)
            for (int nt = 0; nt < 4; ++nt)
                for (int l = 0; l < 64; ++l)
                    for (int q = 0; q < 4; ++q) {
                        const int co = nt * 16 + (l & 15);
                        const int ci = 16 * g + 4 * (l >> 4) + q;
                        *o++ = f.w[((size_t)co * 64 + ci) * 9 + t];
                    }
    assert((size_t)(o - out) == nnl::conv_w(OAZ_FP32));
    memcpy(o + nnl::kConvBias, f.b.data(), 64 * sizeof(float));
}

// The head 1x1 convs as B fragments (h: the heads): [K-half m][piece][lane] x8, lane l supplying
// B[k = 8(l>>4) + e][col n = l&15] for channel 32m + 8(l>>4) + e, columns n = 0 value conv, 1 / 2 policy
// conv planes, 3..15 zero; for OAZ_FP32_SPLIT16 of the column-scaled weights, then 1/s per column.
void pack_head_frags(const FoldedConv& vc, const FoldedConv& pc, int prec, float* h) {
    const bool scaled = prec == OAZ_FP32_SPLIT16;
    float sc[3], inv[3];
    if (scaled) {
        sc[0] = pow2_scale(vc.w.data(), 64, 1, &inv[0]);
        sc[1] = pow2_scale(pc.w.data(), 64, 1, &inv[1]);
        sc[2] = pow2_scale(pc.w.data() + 64, 64, 1, &inv[2]);
    }
    Cursor16 c{h + nnl::kHeadB};
    for (int m = 0; m < 2; ++m)
        put_frags(c, prec, 1, [&](int, int l, int e) {
            const int ch = 32 * m + 8 * (l >> 4) + e, n = l & 15;
            if (n > 2) return 0.0f;
            const float w = n == 0 ? vc.w[ch] : pc.w[(n - 1) * 64 + ch];
            return scaled ? w * sc[n] : w;
        });
    assert(c.n == 2 * nnl::head_b(prec));
    if (scaled) memcpy(h + nnl::head_inv(prec), inv, sizeof(inv));
}

// First layer. Of the 21 input planes only the 4 bitboards vary over the board; the 16 card planes and
// the blue-to-move plane (constant over the board, common.rs:68-77,32-37) become T[square][c][co] = sum
// over the on-board taps of W[co][plane][tap], with c = card index or 16 for the colour plane.
std::vector<float> first_layer_table(const FoldedConv& f) {
    std::vector<float> T(nnl::kL1TableLen);
    for (int sq = 0; sq < 25; ++sq)
        for (int c = 0; c < 17; ++c) {
            const int plane = c < 16 ? 4 + c : 20;
            for (int co = 0; co < 64; ++co) {
                double acc = 0.0;
                for (int t = 0; t < 9; ++t) {
                    const int r = sq / 5 + t / 3 - 1, cc = sq % 5 + t % 3 - 1;
                    if (r < 0 || r > 4 || cc < 0 || cc > 4) continue;
                    acc += (double)f.w[((size_t)co * 21 + plane) * 9 + t];
                }
                T[((size_t)sq * 17 + c) * 64 + co] = (float)acc;
            }
        }
    return T;
}

// Exact-fp32 encoding (k_nn_sq16, k_nn_x6): the bitboard planes through v_mfma_f32_16x16x4f32 (lane l
// supplies W[co = 16nt + (l&15)][plane l>>4][tap t]), the bias and the table.
void pack_first_layer(const FoldedConv& f, const std::vector<float>& T, float* out) {
    float* o = out + nnl::kL1B;
    for (int t = 0; t < 9; ++t)
        for (int nt = 0; nt < 4; ++nt)
            for (int l = 0; l < 64; ++l) *o++ = f.w[((size_t)(nt * 16 + (l & 15)) * 21 + (l >> 4)) * 9 + t];
    memcpy(out + nnl::kL1Bias, f.b.data(), 64 * sizeof(float));
    memcpy(out + nnl::kL1Table, T.data(), T.size() * sizeof(float));
}

// fp16 MFMA encoding (k_nn_h3, both modes): K block 0 = [piece][N-tile][lane] f16x8, lane l supplying
// A[row co = 16nt + (l&15)][k = 8q + e] (q = l>>4) = piece of s_co W[co][plane q][tap e]; K block 1 per
// square = [square][piece][N-tile][lane] f16x8 with k = 8q + e: e = 0 tap 8 of plane q, e >= 1 the table
// T[sq][c = 7q + e - 1][co] (c < 17); then 1/s[64]. s = 2^k per output channel over all of them
// (max |s w| in [2^14, 2^15)).
void pack_first_layer_f16(const FoldedConv& f, const std::vector<float>& T, float* l1c) {
    float s1[64], inv1[64];
    for (int co = 0; co < 64; ++co) {
        float mx = 0.0f;
        for (int pl = 0; pl < 4; ++pl)
            for (int t = 0; t < 9; ++t) mx = fmaxf(mx, fabsf(f.w[((size_t)co * 21 + pl) * 9 + t]));
        for (int sq = 0; sq < 25; ++sq)
            for (int c = 0; c < 17; ++c) mx = fmaxf(mx, fabsf(T[((size_t)sq * 17 + c) * 64 + co]));
        s1[co] = pow2_scale(&mx, 1, 1, &inv1[co]);
    }
    Cursor16 c{l1c};
    for (int blk = 0; blk < 26; ++blk)  // K block 0, then K block 1 of square blk - 1
        put_frags(c, OAZ_FP32_SPLIT16, 4, [&](int nt, int l, int e) {
            const int co = nt * 16 + (l & 15), q = l >> 4, sq = blk - 1;
            float w = 0.0f;
            if (blk == 0) w = f.w[((size_t)co * 21 + q) * 9 + e];
            else if (e == 0) w = f.w[((size_t)co * 21 + q) * 9 + 8];
            else if (7 * q + e - 1 < 17) w = T[((size_t)sq * 17 + 7 * q + e - 1) * 64 + co];
            return w * s1[co];  // exact scaling
        });
    assert(c.n == 2 * nnl::kL1cInv);
    memcpy(l1c + nnl::kL1cInv, inv1, sizeof(inv1));
}

// The blob of one precision at out[0, nn_packed_floats) (zero on entry).
void pack_blob(const float* raw, const wl::Layout& L, int prec, float* out) {
    const int blocks = L.blocks;
    const FoldedConv f1 = fold(raw, L.tower[0]);
    const std::vector<float> T = first_layer_table(f1);
    pack_first_layer(f1, T, out);
    for (int c = 0; c < 2 * blocks; ++c) {
        float* o = out + nnl::kConvs + (size_t)c * nnl::conv_stride(prec);
        if (prec == OAZ_FP32) pack_conv64_f32(fold(raw, L.tower[1 + c]), o);
        else pack_conv64_x32(fold(raw, L.tower[1 + c]), prec, o);
    }
    float* h = out + nnl::heads(prec, blocks);
    // value head: vh_conv + vh_bn folded, vh_linear1, vh_linear2
    const FoldedConv vc = fold(raw, L.vh_conv);
    const float *l1w = raw + L.vh_linear1.w, *plw = raw + L.ph_linear2.w;
    memcpy(h + nnl::kWv, vc.w.data(), 64 * sizeof(float));
    h[nnl::kBv] = vc.b[0];
    for (int q = 0; q < 25; ++q)  // vh_linear1.weight [64][25], stored transposed [25][64] (coalesced per lane)
        for (int o = 0; o < 64; ++o) h[nnl::kL1w + q * 64 + o] = l1w[o * 25 + q];
    memcpy(h + nnl::kL1b, raw + L.vh_linear1.b, 64 * sizeof(float));  // vh_linear1.bias
    memcpy(h + nnl::kL2w, raw + L.vh_linear2.w, 64 * sizeof(float));  // vh_linear2.weight [1][64]
    h[nnl::kL2b] = raw[L.vh_linear2.b];                               // vh_linear2.bias
    // policy head: policy_conv + policy_bn folded, ph_linear2
    const FoldedConv pc = fold(raw, L.policy_conv);
    memcpy(h + nnl::kWp, pc.w.data(), 128 * sizeof(float));
    h[nnl::kBp] = pc.b[0];
    h[nnl::kBp + 1] = pc.b[1];
    for (int f = 0; f < 50; ++f)  // ph_linear2.weight [50 out][50 in], stored transposed [in][out]
        for (int o = 0; o < 50; ++o) h[nnl::kPlw + f * 50 + o] = plw[o * 50 + f];
    memcpy(h + nnl::kPlb, raw + L.ph_linear2.b, 50 * sizeof(float));  // ph_linear2.bias
    if (prec != OAZ_FP32) pack_head_frags(vc, pc, prec, h);
    if (nnl::has_l1c(prec)) pack_first_layer_f16(f1, T, out + nnl::l1c(prec, blocks));
}

}  // namespace

int oaz_pack_weights(const float* raw, size_t raw_floats, int blocks, int precision, std::vector<float>& out) {
    if (!raw || blocks < 0 || precision < OAZ_FP32 || precision > OAZ_FP32_SPLIT16) return OAZ_PACK_BAD_ARG;
    const wl::Layout L = wl::layout(blocks);
    if (raw_floats != L.total) return OAZ_PACK_RAW_SIZE;
    out.assign(nn_device_floats(blocks, precision), 0.0f);
    pack_blob(raw, L, precision, out.data());
    // k_nn_h3 recomputes fp16-range tiles with the k_nn_x6 body: the OAZ_FP32_SPLIT blob follows
    if (precision == OAZ_FP32_SPLIT16) pack_blob(raw, L, OAZ_FP32_SPLIT, out.data() + nn_packed_floats(blocks, precision));
    return OAZ_PACK_OK;
}
