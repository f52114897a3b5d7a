// oaz_replay_host.cpp — oaz_replay_merge_host: the replay buffer's merge rule on the host (include/onitama_az.h,
// "replay buffer"), and oaz_holdout_pick / oaz_holdout_mask_host: the held-out split's rule on the host ("held-out
// evaluation"). No HIP here, so that this file builds and runs alone (tests/c/replay_merge_main.cpp).
#include <new>
#include <vector>

#include "oaz_holdout_rule.h"
#include "oaz_replay_rule.h"

int oaz_set_err(int code, const char* fmt, ...);  // oaz_host.h (which needs the HIP headers)

extern "C" int oaz_replay_merge_host(const oaz_sample* in, size_t n, oaz_sample* out, uint32_t* mult, size_t* n_out) {
    if ((!in || !out) && n) return oaz_set_err(OAZ_ERR_ARG, "replay_merge_host: null pointer");
    if (n >= ((size_t)1 << 31)) return oaz_set_err(OAZ_ERR_ARG, "replay_merge_host: %zu records (at most 2^31 - 1)", n);
    if (n_out) *n_out = 0;
    if (n == 0) return 0;
    try {
        // groups in the order of their first member: an open-addressed table of group numbers, linear probing
        size_t slots = 2;
        while (slots < 2 * n) slots <<= 1;
        const uint32_t kEmpty = 0xFFFFFFFFu;
        std::vector<uint32_t> table(slots, kEmpty), group(n), rep, count;
        std::vector<ReplayKey> keys;  // per group
        for (size_t i = 0; i < n; ++i) {
            uint32_t w[kReplayKeyWords];
            memcpy(w, &in[i], sizeof(w));
            const ReplayKey k = replay_key(w);
            size_t s = replay_key_hash(k) & (slots - 1);
            while (table[s] != kEmpty && !replay_key_equal(keys[table[s]], k)) s = (s + 1) & (slots - 1);
            if (table[s] == kEmpty) {
                table[s] = (uint32_t)rep.size();
                keys.push_back(k);
                rep.push_back((uint32_t)i);
                count.push_back(0);
            }
            group[i] = table[s];
            ++count[group[i]];
        }
        const size_t G = rep.size();
        // integer sums for the groups of more than one member only
        std::vector<uint32_t> acc_of(G, kEmpty);
        size_t multi = 0;
        for (size_t g = 0; g < G; ++g)
            if (count[g] > 1) acc_of[g] = (uint32_t)multi++;
        std::vector<uint64_t> sum_pi(multi * kReplayPi, 0);
        std::vector<int64_t> sum_z(multi, 0);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t a = acc_of[group[i]];
            if (a == kEmpty) continue;
            for (int j = 0; j < kReplayPi; ++j) sum_pi[(size_t)a * kReplayPi + j] += replay_fix_pi(in[i].pi[j]);
            sum_z[a] += replay_fix_z(in[i].z);
        }
        for (size_t g = 0; g < G; ++g) {
            memcpy(&out[g], &in[rep[g]], sizeof(oaz_sample));  // m == 1: byte for byte; else the representative's state
            const uint32_t a = acc_of[g], m = count[g];
            if (a != kEmpty) {
                for (int j = 0; j < kReplayPi; ++j) out[g].pi[j] = replay_mean_pi(sum_pi[(size_t)a * kReplayPi + j], m);
                out[g].z = replay_mean_z(sum_z[a], m);
            }
            if (mult) mult[g] = m;
        }
        if (n_out) *n_out = G;
    } catch (const std::bad_alloc&) {
        return oaz_set_err(OAZ_ERR_CAPACITY, "replay_merge_host: out of host memory for %zu records", n);
    }
    return 0;
}

// ---- the held-out split on the host (oaz_holdout_rule.h) ---------------------------------------------------
static bool holdout_of(uint64_t seed, const void* state, uint32_t per_65536) {
    uint32_t w[kReplayKeyWords];
    memcpy(w, state, sizeof(w));
    return holdout_pick(seed, replay_key(w), per_65536);
}

extern "C" int oaz_holdout_pick(uint64_t seed, const oaz_state* s, uint32_t per_65536) {
    if (!s) return oaz_set_err(OAZ_ERR_ARG, "holdout_pick: null state");
    if (per_65536 > 65536u) return oaz_set_err(OAZ_ERR_ARG, "holdout_pick: per_65536 %u outside 0 .. 65536", per_65536);
    return holdout_of(seed, s, per_65536) ? 1 : 0;
}

extern "C" int oaz_holdout_mask_host(const oaz_sample* in, size_t n, uint64_t seed, uint32_t per_65536, uint8_t* out) {
    if (per_65536 > 65536u) return oaz_set_err(OAZ_ERR_ARG, "holdout_mask_host: per_65536 %u outside 0 .. 65536", per_65536);
    if ((!in || !out) && n) return oaz_set_err(OAZ_ERR_ARG, "holdout_mask_host: null pointer");
    for (size_t i = 0; i < n; ++i) out[i] = holdout_of(seed, &in[i], per_65536) ? 1 : 0;
    return 0;
}
