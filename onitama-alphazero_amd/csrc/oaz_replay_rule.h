// oaz_replay_rule.h — the replay buffer's merge rule (include/onitama_az.h, "replay buffer"), stated once for
// the host entry (oaz_replay_host.cpp) and the kernels (oaz_replay.hip). Plain C++: builds without HIP.
// Not for fast-math: F rounds half to even and the mean is one correctly rounded double division.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/onitama_az.h"

#if defined(__HIPCC__)
#define OAZ_RULE_FN __host__ __device__ inline
#else
#define OAZ_RULE_FN inline
#endif

constexpr int kReplayKeyWords = 6;  // the 22 key bytes in six 32-bit words, the two pad bytes of the last one 0
constexpr int kReplaySampleWords = (int)(sizeof(oaz_sample) / 4);  // 57: state 6, pi 50, z 1
constexpr int kReplayPi = 50;
static_assert(sizeof(oaz_sample) == 228 && sizeof(oaz_state) == 24, "the record layout the rule is stated on");

struct alignas(8) ReplayKey {
    uint32_t w[kReplayKeyWords];
};

// A record's key from its first six words (oaz_state is kings[2], pawns[2], cards[5], to_move, pad[2]; little
// endian: the pad is the high half of word 5).
OAZ_RULE_FN ReplayKey replay_key(const uint32_t* rec_words) {
    ReplayKey k;
    for (int d = 0; d < kReplayKeyWords - 1; ++d) k.w[d] = rec_words[d];
    k.w[5] = rec_words[5] & 0xFFFFu;
    return k;
}

OAZ_RULE_FN bool replay_key_equal(const ReplayKey& a, const ReplayKey& b) {
    uint32_t diff = 0;
    for (int d = 0; d < kReplayKeyWords; ++d) diff |= a.w[d] ^ b.w[d];
    return diff == 0;
}

// 32 bits of the key, mixed well enough for a power-of-two table (murmur3's word step and finaliser).
OAZ_RULE_FN uint32_t replay_key_hash(const ReplayKey& k) {
    uint32_t h = 0x9E3779B9u;
    for (int d = 0; d < kReplayKeyWords; ++d) {
        uint32_t x = k.w[d] * 0xCC9E2D51u;
        x = (x << 15) | (x >> 17);
        h ^= x * 0x1B873593u;
        h = ((h << 13) | (h >> 19)) * 5u + 0xE6546B64u;
    }
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// F(x) = rint(x * 2^32): the product is exact in double, rint rounds half to even.
OAZ_RULE_FN uint64_t replay_fix_pi(float x) { return (uint64_t)rint((double)x * 4294967296.0); }
OAZ_RULE_FN int64_t replay_fix_z(float x) { return (int64_t)rint((double)x * 4294967296.0); }

// The group's entry from its integer sum: one double division, then the cast's round to nearest even.
OAZ_RULE_FN float replay_mean_pi(uint64_t sum, uint32_t m) { return (float)((double)sum / ((double)m * 4294967296.0)); }
OAZ_RULE_FN float replay_mean_z(int64_t sum, uint32_t m) { return (float)((double)sum / ((double)m * 4294967296.0)); }
