// oaz_weights_layout.h — the canonical weight blob, stated once: the flat fp32 array of the
// network's tensors in tch VarStore creation order (net.rs:101-213), which oaz_load_weights,
// oaz_trainer_set_weights, oaz_ot_read / oaz_ot_write and oaz_random_weights exchange. layout() is
// the only walk over that order; the typed offsets (packer, trainer) and the tensor table (named
// loader, .ot reader and writer, random init) both come out of it. To change the network, edit
// layout() (and the independent restatements the tests compare against: weights.py canonical_layout,
// the oracle). Host-only, header-only, no HIP: tests/c/weights_layout_dump.cpp prints it on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace oaz {
namespace wl {

struct Tensor {
    std::string name;           // '|'-joined, as in the .ot files
    std::vector<size_t> shape;  // the tch shape (net.rs)
    size_t offset, numel;       // floats into the blob
    bool running_stat;          // BN running_mean / running_var: no gradient, no SGD update
    size_t fan_in;              // random init U(+-1/sqrt(fan_in)); 0: a BN tensor, filled with `fill`
    float fill;
};

// Float offsets into the blob.
struct ConvBn {  // conv.{weight [cout][cin][k][k], bias} + bn.{weight, bias, running_mean, running_var}
    size_t w, b, gamma, beta, mean, var;
    size_t cout, cin, k;
};
struct Linear {  // {weight [out][in], bias}
    size_t w, b;
    size_t out, in;
};

struct Layout {
    int blocks = 0;
    std::vector<ConvBn> tower;  // conv_init_1 + bn1, then block i's small_block_conv + small_block_bn, j = 1, 2
    ConvBn vh_conv, policy_conv;
    Linear vh_linear1, vh_linear2, ph_linear2;
    size_t total = 0;
    std::vector<Tensor> tensors;  // creation order
};

inline Layout layout(int blocks, size_t channels = 64, size_t in_planes = 21) {
    Layout L;
    L.blocks = blocks;
    auto add = [&](const std::string& name, std::vector<size_t> shape, size_t fan_in, float fill = 0.0f,
                   bool running_stat = false) {
        size_t numel = 1;
        for (size_t d : shape) numel *= d;
        L.tensors.push_back({name, std::move(shape), L.total, numel, running_stat, fan_in, fill});
        L.total += numel;
        return L.total - numel;
    };
    auto conv_bn = [&](const std::string& conv, const std::string& bn, size_t cout, size_t cin, size_t k) {
        ConvBn c{};
        c.cout = cout, c.cin = cin, c.k = k;
        c.w = add(conv + "|weight", {cout, cin, k, k}, cin * k * k);
        c.b = add(conv + "|bias", {cout}, cin * k * k);
        c.gamma = add(bn + "|weight", {cout}, 0, 1.0f);
        c.beta = add(bn + "|bias", {cout}, 0, 0.0f);
        c.mean = add(bn + "|running_mean", {cout}, 0, 0.0f, true);
        c.var = add(bn + "|running_var", {cout}, 0, 1.0f, true);
        return c;
    };
    auto linear = [&](const std::string& name, size_t out, size_t in) {
        Linear l{};
        l.out = out, l.in = in;
        l.w = add(name + "|weight", {out, in}, in);
        l.b = add(name + "|bias", {out}, in);
        return l;
    };
    const size_t C = channels;
    L.tower.push_back(conv_bn("conv_init_1", "bn1", C, in_planes, 3));
    for (int i = 0; i < blocks; ++i)
        for (int j = 1; j <= 2; ++j) {
            const std::string p = "resnet_" + std::to_string(i) + "|resnet_small_block" + std::to_string(j);
            L.tower.push_back(conv_bn(p + "|small_block_conv", p + "|small_block_bn", C, C, 3));
        }
    L.vh_conv = conv_bn("vh_conv", "vh_bn", 1, C, 1);
    L.vh_linear1 = linear("vh_linear1", C, 25);
    L.vh_linear2 = linear("vh_linear2", 1, C);
    L.policy_conv = conv_bn("policy_conv", "policy_bn", 2, C, 1);
    L.ph_linear2 = linear("ph_linear2", 50, 50);
    return L;
}

// The running statistics as maximal runs of the blob, in blob order: a layer's running_mean and
// running_var are adjacent, so one run each per tower conv, then the value head's, the policy head's.
struct Run {
    size_t offset, len;
};
inline std::vector<Run> running_stat_runs(const Layout& L) {
    std::vector<Run> r;
    for (const Tensor& t : L.tensors) {
        if (!t.running_stat) continue;
        if (!r.empty() && r.back().offset + r.back().len == t.offset) r.back().len += t.numel;
        else r.push_back({t.offset, t.numel});
    }
    return r;
}

// 1 where SGD (and weight decay) applies: everything but the running statistics.
inline std::vector<uint8_t> sgd_mask(const Layout& L) {
    std::vector<uint8_t> m(L.total, 1);
    for (const Run& r : running_stat_runs(L))
        for (size_t i = 0; i < r.len; ++i) m[r.offset + i] = 0;
    return m;
}

}  // namespace wl
}  // namespace oaz
