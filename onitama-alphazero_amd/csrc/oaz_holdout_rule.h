// oaz_holdout_rule.h — the held-out split (include/onitama_az.h, "held-out evaluation"),
// stated once for the host entries (oaz_replay_host.cpp) and the kernel (oaz_replay.hip). Plain C++: builds
// without HIP.
//
// A record is held out as a function of its position only: the key is the replay buffer's (replay_key: the 22
// state bytes in six words, the pad bytes 0), so every copy of a position, in every iteration of a replay
// window, and a merged record and its members, fall on the same side.
//   a = philox(seed; k0, k1, k2, k3)
//   b = philox(a.w0 | a.w1 << 32; k4, k5, "HOLD", 0)
//   held out iff (b.w0 & 0xFFFF) < H, H in 0 .. 65536 (0: none, 65536: all)
#pragma once

#include "oaz_device.h"
#include "oaz_replay_rule.h"

constexpr uint32_t kHoldoutTag = 0x484F4C44u;  // "HOLD"

OAZ_RULE_FN bool holdout_pick(uint64_t seed, const ReplayKey& k, uint32_t per_65536) {
    const oaz::u32x4 a = oaz::philox(seed, k.w[0], k.w[1], k.w[2], k.w[3]);
    const oaz::u32x4 b = oaz::philox((uint64_t)a.x | ((uint64_t)a.y << 32), k.w[4], k.w[5], kHoldoutTag, 0u);
    return (b.x & 0xFFFFu) < per_65536;
}
