// oaz_replay.hip — the device replay buffer (include/onitama_az.h, "replay buffer"): a
// window of segments kept contiguous on the device, and the merged view of it, one launch per phase:
//   key     pack the 22 key bytes of every record and hash them
//   insert  an open-addressed table of arrival indices; per key the smallest index wins (atomicCAS, atomicMin)
//   lookup  rep_of[i] = the table's index for record i's key; flag[i] = (rep_of[i] == i)
//   scan    flags to output positions, in tiles of 4,096 with a second level over the tile sums
//   group   every record's group and its rank in it (one atomicAdd), the counts scanned to member-list starts,
//           the member lists filled (a counting sort by group)
//   emit    one wave per group: a group of one copies its record; else the lanes stride over the members, sum
//           F(pi), F(z) in 64-bit integers in registers, the wave adds the lanes up and writes the means
// No kernel waits for another workgroup; a probe loop is bounded by the slot count and reports through `err`.
#include <hip/hip_runtime.h>

#include <vector>

#include "oaz_holdout_rule.h"
#include "oaz_host.h"
#include "oaz_replay_rule.h"

namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr int kThreads = 256;
constexpr int kTilePer = 16;                       // elements per thread of a scan tile
constexpr int kTile = kThreads * kTilePer;         // 4,096
constexpr int kTopThreads = 1024;                  // the second level's one workgroup
enum { ERR_TABLE_FULL = 1, ERR_KEY_MISSING = 2 };
enum { CTR_ERR = 0, CTR_TOTAL = 1, CTR_MAXMULT = 2, CTR_WORDS = 4 };  // uint32 words; probes: the uint64 after them

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void __launch_bounds__(kThreads) k_replay_key(const uint32_t* rec, uint32_t n, ReplayKey* keys, uint32_t* hash) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const ReplayKey k = replay_key(rec + (size_t)i * kReplaySampleWords);
    keys[i] = k;
    hash[i] = replay_key_hash(k);
}

// The slot of record i's key: an empty slot is claimed with i, a taken one names a record whose key is compared.
// A slot's key never changes once it is claimed (only atomicMin among records of that key writes it again), so
// a lost CAS re-reads the slot and compares like any other taken slot.
__global__ void __launch_bounds__(kThreads) k_replay_insert(const ReplayKey* keys, const uint32_t* hash, uint32_t n,
                                                            uint32_t* table, uint32_t mask, uint32_t* ctr,
                                                            unsigned long long* probes) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long cmp = 0;
    if (i < n) {
        const ReplayKey k = keys[i];
        uint32_t s = hash[i] & mask;
        bool done = false;
        for (uint32_t p = 0; p <= mask && !done; ++p, s = (s + 1) & mask) {
            uint32_t cur = __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kEmpty) {
                cur = atomicCAS(&table[s], kEmpty, i);
                if (cur == kEmpty) {
                    done = true;
                    break;
                }
            }
            ++cmp;
            if (cur < n && replay_key_equal(keys[cur], k)) {
                atomicMin(&table[s], i);
                done = true;
            }
        }
        if (!done) atomicOr(&ctr[CTR_ERR], (uint32_t)ERR_TABLE_FULL);
    }
    cmp = wave_sum(cmp);
    if ((threadIdx.x & 63) == 0 && cmp) atomicAdd(probes, cmp);
}

__global__ void __launch_bounds__(kThreads) k_replay_lookup(const ReplayKey* keys, const uint32_t* hash, uint32_t n,
                                                            const uint32_t* table, uint32_t mask, uint32_t* rep_of,
                                                            uint32_t* flag, uint32_t* ctr, unsigned long long* probes) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long cmp = 0;
    if (i < n) {
        const ReplayKey k = keys[i];
        uint32_t s = hash[i] & mask, rep = kEmpty;
        for (uint32_t p = 0; p <= mask; ++p, s = (s + 1) & mask) {
            const uint32_t cur = table[s];
            if (cur >= n) break;  // empty: the key is not in the table
            ++cmp;
            if (replay_key_equal(keys[cur], k)) {
                rep = cur;
                break;
            }
        }
        if (rep == kEmpty) {
            atomicOr(&ctr[CTR_ERR], (uint32_t)ERR_KEY_MISSING);
            rep = i;  // in range, whatever follows
        }
        rep_of[i] = rep;
        flag[i] = rep == i;
    }
    cmp = wave_sum(cmp);
    if ((threadIdx.x & 63) == 0 && cmp) atomicAdd(probes, cmp);
}

// ---- exclusive scan of n uint32 in tiles (the shape of k_samples_scan, oaz_kernels.hip, per tile) ----------
// Level 1: every thread sums its run of kTilePer consecutive elements, the workgroup scans the runs in LDS, and
// every element's position inside the tile goes to out; the tile's sum to tile_sum.
__global__ void __launch_bounds__(kThreads) k_replay_scan_tiles(const uint32_t* in, uint32_t n, uint32_t* out,
                                                                uint32_t* tile_sum) {
    const size_t base = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kTilePer;
    uint32_t v[kTilePer], sum = 0;
#pragma unroll
    for (int k = 0; k < kTilePer; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        sum += v[k];
    }
    __shared__ uint32_t run[kThreads];
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {  // inclusive Hillis-Steele scan of the runs
        const uint32_t o = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0u;
        __syncthreads();
        run[threadIdx.x] += o;
        __syncthreads();
    }
    uint32_t pos = run[threadIdx.x] - sum;
#pragma unroll
    for (int k = 0; k < kTilePer; ++k) {
        if (base + k < n) out[base + k] = pos;
        pos += v[k];
    }
    if (threadIdx.x == kThreads - 1) tile_sum[blockIdx.x] = run[kThreads - 1];
}

// Level 2, one workgroup: the tile sums to tile offsets in place, and the grand total to *total.
__global__ void __launch_bounds__(kTopThreads) k_replay_scan_top(uint32_t* tile_sum, uint32_t tiles, uint32_t* total) {
    const uint32_t per = (tiles + kTopThreads - 1) / kTopThreads;
    const uint32_t t0 = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; ++t) sum += tile_sum[t];
    __shared__ uint32_t run[kTopThreads];
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kTopThreads; d <<= 1) {
        const uint32_t o = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0u;
        __syncthreads();
        run[threadIdx.x] += o;
        __syncthreads();
    }
    uint32_t pos = run[threadIdx.x] - sum;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t s = tile_sum[t];
        tile_sum[t] = pos;
        pos += s;
    }
    if (threadIdx.x == kTopThreads - 1) *total = run[kTopThreads - 1];
}

// Level 3: every element's position in the whole array.
__global__ void __launch_bounds__(kThreads) k_replay_scan_add(uint32_t* out, uint32_t n, const uint32_t* tile_off) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] += tile_off[i / kTile];
}

// Every record's group (its representative's output position) and its rank among the group's members, in
// whatever order the adds land (the sums are integers); a representative also names itself as the group's.
__global__ void __launch_bounds__(kThreads) k_replay_group(const uint32_t* rep_of, const uint32_t* pos, uint32_t n,
                                                           uint32_t* group, uint32_t* rank, uint32_t* count,
                                                           uint32_t* rep_idx) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rep_of[i], g = pos[r];
    group[i] = g;
    rank[i] = atomicAdd(&count[g], 1u);
    if (r == i) rep_idx[g] = i;
}

__global__ void __launch_bounds__(kThreads) k_replay_members(const uint32_t* group, const uint32_t* rank, uint32_t n,
                                                             const uint32_t* start, uint32_t* members) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) members[start[group[i]] + rank[i]] = i;
}

__global__ void __launch_bounds__(kThreads) k_replay_emit(const uint32_t* rec, uint32_t groups, const uint32_t* rep_idx,
                                                          const uint32_t* count, const uint32_t* start,
                                                          const uint32_t* members, uint32_t* out, uint32_t* ctr) {
    const uint32_t g = blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
    if (g >= groups) return;  // (whole waves leave: a wave is one group)
    const int l = threadIdx.x & 63;
    const uint32_t m = count[g];
    const uint32_t* src = rec + (size_t)rep_idx[g] * kReplaySampleWords;
    uint32_t* dst = out + (size_t)g * kReplaySampleWords;
    if (m == 1) {
        if (l < kReplaySampleWords) dst[l] = src[l];
        return;
    }
    unsigned long long acc[kReplayPi];
    long long zacc = 0;
#pragma unroll
    for (int j = 0; j < kReplayPi; ++j) acc[j] = 0;
    const uint32_t* mem = members + start[g];
    for (uint32_t k = (uint32_t)l; k < m; k += 64) {
        const float* f = reinterpret_cast<const float*>(rec + (size_t)mem[k] * kReplaySampleWords + kReplayKeyWords);
#pragma unroll
        for (int j = 0; j < kReplayPi; ++j) acc[j] += replay_fix_pi(f[j]);
        zacc += replay_fix_z(f[kReplayPi]);
    }
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < kReplayPi; ++j) {
        const unsigned long long s = wave_sum(acc[j]);
        if (l == j) mine = replay_mean_pi(s, m);
    }
    const long long sz = (long long)wave_sum((unsigned long long)zacc);  // two's complement: the signed sum
    if (l == kReplayPi) mine = replay_mean_z(sz, m);
    if (l <= kReplayPi) dst[kReplayKeyWords + l] = __float_as_uint(mine);
    if (l < kReplayKeyWords) dst[l] = src[l];
    if (l == 0 && m > ctr[CTR_MAXMULT]) atomicMax(&ctr[CTR_MAXMULT], m);
}

struct Segment {
    size_t n;
    int64_t tag;
};

}  // namespace

struct oaz_replay {
    oaz_replay_config cfg;
    int device = 0;
    Stream stream;
    DevBuf<oaz_sample> store[2];  // the window's records in store[cur], contiguous, in arrival order
    int cur = 0;
    std::vector<Segment> segs;
    size_t records = 0;
    uint64_t appended = 0, evicted = 0, unique = 0, max_mult = 0, probes = 0;
    // merge scratch, grow-only
    DevBuf<ReplayKey> keys;
    DevBuf<uint32_t> hash, table, rep_of, flag, pos, group, rank, members, tile_sum, rep_idx, count, start;
    DevBuf<oaz_sample> merged;
    DevBuf<uint32_t> ctr;  // CTR_WORDS uint32 and one uint64
    Event ev[OAZ_REPLAY_PHASES + 1];
    double phase_ms[OAZ_REPLAY_PHASES] = {0, 0, 0, 0, 0, 0};
};

extern "C" void oaz_replay_config_default(oaz_replay_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->capacity = 180000;  // TrainConfig.buffer_size, train.rs:128
    c->window = 1;
}

extern "C" oaz_replay* oaz_replay_create(const oaz_replay_config* cfg) {
    if (!cfg || cfg->capacity == 0 || cfg->capacity >= (1ull << 31) || cfg->window < 1) {
        oaz_set_err(OAZ_ERR_ARG, "replay_create: capacity in [1, 2^31) and window >= 1");
        return nullptr;
    }
    if (oaz_check_device("replay_create", cfg->device)) return nullptr;
    DeviceScope scope(cfg->device);
    if (scope.rc != hipSuccess) {
        oaz_set_err(OAZ_ERR_HIP, "replay_create: hipSetDevice(%d): %s", cfg->device, hipGetErrorString(scope.rc));
        return nullptr;
    }
    oaz_replay* r = new oaz_replay;
    r->cfg = *cfg;
    r->device = cfg->device;
    int rc = r->stream.create();
    if (!rc) rc = r->ctr.alloc(CTR_WORDS + 2);
    for (int k = 0; k <= OAZ_REPLAY_PHASES && !rc; ++k) rc = r->ev[k].create(hipEventDefault);
    if (rc) {
        delete r;
        return nullptr;
    }
    return r;
}

extern "C" void oaz_replay_destroy(oaz_replay* r) {
    if (!r) return;
    DeviceScope scope(r->device);
    (void)r->stream.sync();
    delete r;
}

// What the window rule leaves of the present segments once a segment of n records has arrived: the number of
// oldest segments dropped and their records.
static void window_after(const oaz_replay* r, size_t n, size_t* drop_segs, size_t* drop_recs) {
    size_t segs = r->segs.size() + 1, recs = r->records + n, k = 0, gone = 0;
    while (segs > (size_t)r->cfg.window) gone += r->segs[k++].n, --segs;
    while (recs - gone > r->cfg.capacity && segs > 1) gone += r->segs[k++].n, --segs;
    *drop_segs = k;
    *drop_recs = gone;
}

static int replay_append(oaz_replay* r, const oaz_sample* src, size_t n, int64_t tag, hipMemcpyKind kind, const char* who) {
    if (!r || (!src && n)) return oaz_set_err(OAZ_ERR_ARG, "%s: null pointer", who);
    if (n > r->cfg.capacity)
        return oaz_set_err(OAZ_ERR_CAPACITY, "%s: segment %lld holds %zu records, the buffer %llu", who, (long long)tag, n,
                           (unsigned long long)r->cfg.capacity);
    OAZ_ON_DEVICE(r->device);
    size_t drop_segs = 0, drop_recs = 0;
    window_after(r, n, &drop_segs, &drop_recs);
    const size_t keep = r->records - drop_recs, total = keep + n;
    if (keep == 0) {  // nothing survives: the segment starts the buffer it is in
        if (int rc = r->store[r->cur].reserve(total)) return rc;
    } else if (drop_recs || total > r->store[r->cur].size()) {  // the survivors move to the front of the other buffer
        DevBuf<oaz_sample>& to = r->store[r->cur ^ 1];
        if (int rc = to.reserve(total)) return rc;
        if (keep)
            HIP_TRY(hipMemcpyAsync(to.get(), r->store[r->cur].get() + drop_recs, keep * sizeof(oaz_sample),
                                   hipMemcpyDeviceToDevice, r->stream));
        r->cur ^= 1;
    }
    if (n) HIP_TRY(hipMemcpyAsync(r->store[r->cur].get() + keep, src, n * sizeof(oaz_sample), kind, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->segs.erase(r->segs.begin(), r->segs.begin() + (ptrdiff_t)drop_segs);
    r->segs.push_back({n, tag});
    r->records = total;
    r->appended += n;
    r->evicted += drop_recs;
    return 0;
}

extern "C" int oaz_replay_append_host(oaz_replay* r, const oaz_sample* host, size_t n, int64_t tag) {
    return replay_append(r, host, n, tag, hipMemcpyHostToDevice, "replay_append_host");
}

extern "C" int oaz_replay_append_device(oaz_replay* r, const oaz_sample* dev, size_t n, int64_t tag) {
    return replay_append(r, dev, n, tag, hipMemcpyDeviceToDevice, "replay_append_device");
}

extern "C" int oaz_replay_append_engine(oaz_replay* r, oaz_engine* eng, int64_t tag, size_t* n_out) {
    if (!r || !eng) return oaz_set_err(OAZ_ERR_ARG, "replay_append_engine: null pointer");
    const oaz_sample* src = nullptr;
    size_t n = 0;
    int dev = -1;
    if (int rc = oaz_engine_samples_peek(eng, &src, &n, &dev)) return rc;
    if (dev != r->device)
        return oaz_set_err(OAZ_ERR_ARG, "replay_append_engine: segment %lld: the engine is on device %d, the buffer on %d",
                           (long long)tag, dev, r->device);
    if (int rc = replay_append(r, src, n, tag, hipMemcpyDeviceToDevice, "replay_append_engine")) return rc;
    if (n_out) *n_out = n;
    return oaz_engine_samples_consume(eng, n);
}

static inline unsigned grid_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

// Exclusive scan of in[n] to out[n] on the buffer's stream; the total lands in *total (device).
static int replay_scan(oaz_replay* r, const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* total) {
    const uint32_t tiles = grid_of(n, kTile);
    hipLaunchKernelGGL(k_replay_scan_tiles, dim3(tiles), dim3(kThreads), 0, r->stream, in, n, out, r->tile_sum.get());
    hipLaunchKernelGGL(k_replay_scan_top, dim3(1), dim3(kTopThreads), 0, r->stream, r->tile_sum.get(), tiles, total);
    hipLaunchKernelGGL(k_replay_scan_add, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, r->stream, out, n,
                       r->tile_sum.get());
    HIP_TRY(hipGetLastError());
    return 0;
}

// The merged view of the window's n > 0 records into r->merged / r->count.
static int replay_merge(oaz_replay* r, uint32_t n) {
    uint64_t slots = r->cfg.table_slots;
    if (slots == 0) {
        slots = 2;
        while (slots < 2ull * n) slots <<= 1;
    } else if ((slots & (slots - 1)) || slots <= n) {
        return oaz_set_err(OAZ_ERR_ARG, "replay_view: table_slots %u is not a power of two above the view's %u records",
                           r->cfg.table_slots, n);
    }
    const uint32_t mask = (uint32_t)(slots - 1);
    HIP_TRY(hipStreamSynchronize(r->stream));  // before a reserve frees what the last merge used
    if (int rc = r->keys.reserve(n)) return rc;
    for (DevBuf<uint32_t>* b : {&r->hash, &r->rep_of, &r->flag, &r->pos, &r->group, &r->rank, &r->members})
        if (int rc = b->reserve(n)) return rc;
    if (int rc = r->table.reserve(slots)) return rc;
    if (int rc = r->tile_sum.reserve(grid_of(n, kTile))) return rc;
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(r->store[r->cur].get());
    uint32_t* ctr = r->ctr.get();
    unsigned long long* probes = reinterpret_cast<unsigned long long*>(ctr + CTR_WORDS);
    hipStream_t st = r->stream;
    const dim3 grid(grid_of(n, kThreads)), block(kThreads);
    HIP_TRY(hipEventRecord(r->ev[0], st));  // (the key phase's time includes the table's fill)
    HIP_TRY(hipMemsetAsync(ctr, 0, (CTR_WORDS + 2) * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(r->table.get(), 0xFF, slots * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_replay_key, grid, block, 0, st, rec, n, r->keys.get(), r->hash.get());
    HIP_TRY(hipEventRecord(r->ev[1], st));
    hipLaunchKernelGGL(k_replay_insert, grid, block, 0, st, r->keys.get(), r->hash.get(), n, r->table.get(), mask, ctr, probes);
    HIP_TRY(hipEventRecord(r->ev[2], st));
    hipLaunchKernelGGL(k_replay_lookup, grid, block, 0, st, r->keys.get(), r->hash.get(), n, r->table.get(), mask,
                       r->rep_of.get(), r->flag.get(), ctr, probes);
    HIP_TRY(hipEventRecord(r->ev[3], st));
    if (int rc = replay_scan(r, r->flag.get(), n, r->pos.get(), ctr + CTR_TOTAL)) return rc;
    HIP_TRY(hipEventRecord(r->ev[4], st));
    uint32_t h[CTR_WORDS + 2];
    HIP_TRY(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(&r->probes, h + CTR_WORDS, sizeof(uint64_t));
    const uint32_t groups = h[CTR_TOTAL];
    if (h[CTR_ERR] || groups == 0 || groups > n)
        return oaz_set_err(OAZ_ERR_INTERNAL, "replay_view: the key table failed (code %u, %u groups of %u records in %llu slots)",
                           h[CTR_ERR], groups, n, (unsigned long long)slots);
    for (DevBuf<uint32_t>* b : {&r->rep_idx, &r->count, &r->start})
        if (int rc = b->reserve(groups)) return rc;
    if (int rc = r->merged.reserve(groups)) return rc;
    HIP_TRY(hipMemsetAsync(r->count.get(), 0, (size_t)groups * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_replay_group, grid, block, 0, st, r->rep_of.get(), r->pos.get(), n, r->group.get(), r->rank.get(),
                       r->count.get(), r->rep_idx.get());
    if (int rc = replay_scan(r, r->count.get(), groups, r->start.get(), ctr + CTR_TOTAL)) return rc;
    hipLaunchKernelGGL(k_replay_members, grid, block, 0, st, r->group.get(), r->rank.get(), n, r->start.get(), r->members.get());
    HIP_TRY(hipEventRecord(r->ev[5], st));
    hipLaunchKernelGGL(k_replay_emit, dim3(grid_of(groups, kThreads / 64)), block, 0, st, rec, groups, r->rep_idx.get(),
                       r->count.get(), r->start.get(), r->members.get(), reinterpret_cast<uint32_t*>(r->merged.get()), ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->ev[6], st));
    HIP_TRY(hipMemcpyAsync(h, ctr, CTR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    r->unique = groups;
    r->max_mult = h[CTR_MAXMULT] > 1 ? h[CTR_MAXMULT] : 1;
    for (int k = 0; k < OAZ_REPLAY_PHASES; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r->ev[k], r->ev[k + 1]));
        r->phase_ms[k] = ms;
    }
    return 0;
}

extern "C" int oaz_replay_view(oaz_replay* r, int merge, const oaz_sample** dev, size_t* n, const uint32_t** dev_mult) {
    if (!r || !dev || !n || (merge & ~1)) return oaz_set_err(OAZ_ERR_ARG, "replay_view: bad arguments");
    OAZ_ON_DEVICE(r->device);
    *dev = nullptr;
    *n = 0;
    if (dev_mult) *dev_mult = nullptr;
    if (merge && r->records) {
        if (int rc = replay_merge(r, (uint32_t)r->records)) return rc;
        *dev = r->merged.get();
        *n = (size_t)r->unique;
        if (dev_mult) *dev_mult = r->count.get();
        return 0;
    }
    if (merge) r->unique = 0, r->max_mult = 0, r->probes = 0;
    HIP_TRY(hipStreamSynchronize(r->stream));
    *dev = r->store[r->cur].get();
    *n = r->records;
    return 0;
}

extern "C" int oaz_replay_fetch(oaz_replay* r, int merge, oaz_sample* out, uint32_t* mult, size_t cap, size_t* n_out) {
    if (!r || (!out && cap)) return oaz_set_err(OAZ_ERR_ARG, "replay_fetch: bad arguments");
    const oaz_sample* dev = nullptr;
    const uint32_t* dm = nullptr;
    size_t n = 0;
    if (int rc = oaz_replay_view(r, merge, &dev, &n, &dm)) return rc;
    if (n_out) *n_out = n;
    if (n > cap) return oaz_set_err(OAZ_ERR_CAPACITY, "replay_fetch: the view holds %zu records, the caller's array %zu", n, cap);
    if (n == 0) return 0;
    OAZ_ON_DEVICE(r->device);
    HIP_TRY(hipMemcpyAsync(out, dev, n * sizeof(oaz_sample), hipMemcpyDeviceToHost, r->stream));
    if (mult && dm) HIP_TRY(hipMemcpyAsync(mult, dm, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (mult && !dm)
        for (size_t i = 0; i < n; ++i) mult[i] = 1;
    return 0;
}

extern "C" int oaz_replay_stats_get(oaz_replay* r, oaz_replay_stats* o) {
    if (!r || !o) return oaz_set_err(OAZ_ERR_ARG, "replay_stats: null");
    memset(o, 0, sizeof(*o));
    o->segments = r->segs.size();
    o->records = r->records;
    o->unique = r->unique;
    o->max_mult = r->max_mult;
    o->appended = r->appended;
    o->evicted = r->evicted;
    o->probes = r->probes;
    return 0;
}

extern "C" int oaz_replay_merge_times(oaz_replay* r, double ms[OAZ_REPLAY_PHASES]) {
    if (!r || !ms) return oaz_set_err(OAZ_ERR_ARG, "replay_merge_times: null");
    for (int k = 0; k < OAZ_REPLAY_PHASES; ++k) ms[k] = r->phase_ms[k];
    return 0;
}

// ---- the held-out split over device-resident records (oaz_holdout_rule.h) ----------------------------------
// One thread per record: its six key words, two Philox blocks, one byte. The records are only read.
namespace {
__global__ void __launch_bounds__(kThreads) k_holdout_mask(const uint32_t* rec, size_t n, uint64_t seed, uint32_t per_65536,
                                                           uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    out[i] = holdout_pick(seed, replay_key(rec + i * kReplaySampleWords), per_65536) ? 1 : 0;
}
}  // namespace

extern "C" int oaz_holdout_mask(const oaz_sample* dev, size_t n, uint64_t seed, uint32_t per_65536, int device,
                                uint8_t* host_out) {
    if (per_65536 > 65536u) return oaz_set_err(OAZ_ERR_ARG, "holdout_mask: per_65536 %u outside 0 .. 65536", per_65536);
    if ((!dev || !host_out) && n) return oaz_set_err(OAZ_ERR_ARG, "holdout_mask: null pointer");
    if (n >= ((size_t)1 << 31)) return oaz_set_err(OAZ_ERR_ARG, "holdout_mask: %zu records (at most 2^31 - 1)", n);
    if (n == 0) return 0;
    if (int rc = oaz_check_device("holdout_mask", device)) return rc;
    OAZ_ON_DEVICE(device);
    Stream st;  // (declared before the buffer: destroyed, and so waited for, after it is freed by a synchronous hipFree)
    DevBuf<uint8_t> out;
    if (int rc = st.create()) return rc;
    if (int rc = out.alloc(n)) return rc;
    hipLaunchKernelGGL(k_holdout_mask, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       reinterpret_cast<const uint32_t*>(dev), n, seed, per_65536, out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_out, out, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
