// replay_merge_main.cpp — oaz_replay_merge_host in a program of its own, for a host sanitizer build
// (tests/test_replay.py builds it with csrc/oaz_replay_host.cpp alone, -fsanitize=address,undefined, and runs
// it on the CPU). The mixed input: 40 keys with multiplicities 1 .. 300, shuffled; the arrays are exactly as
// large as the entry may touch, so a write or read past them is reported. Prints "replay_merge_host OK".
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/onitama_az.h"

int oaz_set_err(int code, const char* fmt, ...) {  // the library's is in oaz_engine.cpp
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t next_u32() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 32);
}

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    std::vector<oaz_sample> in;
    const float zs[5] = {-1.f, 0.f, 1.f, 0.5f, -0.25f};
    size_t singles = 0;
    for (uint32_t k = 0; k < 40; ++k) {
        const uint32_t m = k < 8 ? 1 : 1 + next_u32() % 300;
        singles += m == 1;
        for (uint32_t c = 0; c < m; ++c) {
            oaz_sample s;
            memset(&s, 0, sizeof(s));
            s.state.kings[0] = (k + 1) << 7;
            s.state.cards[0] = (uint8_t)(k % 16);
            s.state.to_move = (uint8_t)(k & 1);
            s.state.pad[0] = (uint8_t)next_u32();  // not part of the key
            float sum = 0.f;
            for (int j = 0; j < 50; ++j) sum += s.pi[j] = next_u32() % 3 ? 0.f : (float)(next_u32() >> 8);
            for (int j = 0; j < 50; ++j) s.pi[j] = sum > 0.f ? s.pi[j] / sum : 0.02f;
            s.z = zs[next_u32() % 5];
            in.push_back(s);
        }
    }
    for (size_t i = in.size(); i > 1; --i) {  // Fisher-Yates
        const size_t j = next_u32() % i;
        oaz_sample t = in[i - 1];
        in[i - 1] = in[j];
        in[j] = t;
    }
    const size_t n = in.size();
    std::vector<oaz_sample> out(n), again(n);
    std::vector<uint32_t> mult(n), mult2(n);
    size_t g = 0, g2 = 0;
    CHECK(oaz_replay_merge_host(in.data(), n, out.data(), mult.data(), &g) == 0 && g == 40);
    size_t total = 0, ones = 0;
    for (size_t i = 0; i < g; ++i) total += mult[i], ones += mult[i] == 1;
    CHECK(total == n && ones >= singles);
    for (size_t i = 0; i < g; ++i) {
        float sum = 0.f;
        for (int j = 0; j < 50; ++j) sum += out[i].pi[j];
        CHECK(sum > 0.999f && sum < 1.001f && out[i].z >= -1.f && out[i].z <= 1.f);
    }
    // merging the merged buffer changes nothing (every group is then of one), with arrays of exactly g records
    out.resize(g);
    out.shrink_to_fit();
    again.resize(g);
    again.shrink_to_fit();
    mult2.resize(g);
    mult2.shrink_to_fit();
    CHECK(oaz_replay_merge_host(out.data(), g, again.data(), mult2.data(), &g2) == 0 && g2 == g);
    CHECK(memcmp(out.data(), again.data(), g * sizeof(oaz_sample)) == 0);
    for (size_t i = 0; i < g; ++i) CHECK(mult2[i] == 1);
    // the optional outputs, n == 0, and the argument check
    std::vector<oaz_sample> third(n);
    CHECK(oaz_replay_merge_host(in.data(), n, third.data(), nullptr, nullptr) == 0);
    CHECK(memcmp(out.data(), third.data(), g * sizeof(oaz_sample)) == 0);
    CHECK(oaz_replay_merge_host(nullptr, 0, nullptr, nullptr, &g2) == 0 && g2 == 0);
    CHECK(oaz_replay_merge_host(nullptr, 1, out.data(), nullptr, nullptr) == OAZ_ERR_ARG);
    printf("replay_merge_host OK: %zu records, %zu groups\n", n, g);
    return 0;
}
