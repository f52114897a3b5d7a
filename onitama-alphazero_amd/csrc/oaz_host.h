// oaz_host.h — host-side helpers shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/onitama_az.h"

// Records the thread-local error message returned by oaz_last_error(); returns `code`.
int oaz_set_err(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return oaz_set_err(OAZ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                             \
    } while (0)

// An entry point's device: `device` is current for the call and the calling thread's current device is
// restored on return (every C-ABI entry point that touches the GPU; include/onitama_az.h, Threading).
struct DeviceScope {
    int prev = -1;
    hipError_t rc;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        rc = hipSetDevice(device);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define OAZ_ON_DEVICE(dev)       \
    DeviceScope dev_scope_(dev); \
    HIP_TRY(dev_scope_.rc)

// "No HIP device visible" and "device d out of range" for the entry points that take a device number.
// OAZ_ERR_NO_DEVICE for the first; `range_code` for the second (OAZ_ERR_ARG, the trainer OAZ_ERR_NO_DEVICE).
inline int oaz_check_device(const char* who, int device, int range_code = OAZ_ERR_ARG) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return oaz_set_err(OAZ_ERR_NO_DEVICE, "%s: no HIP device visible", who);
    if (device < 0 || device >= n) return oaz_set_err(range_code, "%s: device %d out of range (%d visible)", who, device, n);
    return 0;
}

// What every entry point asks of a root: to_move 0 or 1, cards 0..15 and, with `squares`, bitboards that hold
// squares 0..24 only (the searches' kernels index the attack table by square and by card).
inline bool oaz_root_ok(const oaz_state& s, bool squares = true) {
    return !(s.to_move & ~1) && (s.cards[0] | s.cards[1] | s.cards[2] | s.cards[3] | s.cards[4]) <= 15 &&
           !(squares && ((s.kings[0] | s.kings[1] | s.pawns[0] | s.pawns[1]) & 0x7Fu));
}

// A search_time_ns budget in ticks of the device's constant-rate clock (hipDeviceAttributeWallClockRate, kHz),
// at most `most`.
inline uint64_t oaz_budget_ticks(int64_t search_time_ns, int wall_khz, double most) {
    const double ticks = (double)search_time_ns * (double)wall_khz * 1e-6;
    return ticks < most ? (uint64_t)ticks : (uint64_t)most;
}

// ---- owners of device resources ----------------------------------------------------------------------
// Movable, not copyable; a default-made one holds nothing and its destructor does nothing. The destructors
// run on the calling thread's current device, so whoever deletes a holder of owners is on the holder's
// device (DeviceScope before delete) and has synchronised the streams the resources were used on. Members
// are destroyed in reverse declaration order: a holder declares its streams first (destroyed last), then
// its buffers, then its events (destroyed first). Holders of static lifetime are made with `new` and never
// deleted: a destructor that calls hipFree while the HIP runtime unloads at process exit can hang.

// A device array of `size()` elements of T.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    ~DevBuf() { reset(); }
    // hipFree waits for the whole device: not for the create, play and read-back path of a live owner.
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // `count` elements, contents undefined (a zero count still allocates 16 bytes: get() is never null).
    int alloc(size_t count) {
        reset();
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16));
        p_ = static_cast<T*>(q);
        n_ = count;
        return 0;
    }
    // Grow-only: at least `count` elements; growing drops the contents. The old buffer is freed, so the
    // caller first synchronises the stream that may still use it.
    int reserve(size_t count) { return count <= n_ ? 0 : alloc(count); }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    operator T*() const { return p_; }  // kernel arguments and offsets read as with a raw pointer
};

// A non-blocking stream. The destructor waits for the stream's work before it destroys the stream, so a
// stream declared after a buffer (destroyed before it) is done with the buffer when that is freed.
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    ~Stream() {
        (void)sync();
        if (s_) (void)hipStreamDestroy(s_);
    }
    int create() {
        HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return 0;
    }
    // Waits for the stream's work (nothing to wait for before create()).
    hipError_t sync() const { return s_ ? hipStreamSynchronize(s_) : hipSuccess; }
    operator hipStream_t() const { return s_; }
};

class Event {
    hipEvent_t ev_ = nullptr;

public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    ~Event() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    int create(unsigned flags = hipEventDisableTiming) {
        HIP_TRY(hipEventCreateWithFlags(&ev_, flags));
        return 0;
    }
    operator hipEvent_t() const { return ev_; }
};

// 256-byte aligned sections of one device allocation. The same take() calls run twice: on Carver{nullptr}
// they only add up (`off` is then the allocation to make), on Carver{allocation} they return the sections.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// Page-locked host memory (hipHostMalloc): what an asynchronous copy may read or write while the host goes on.
template <class T>
class PinnedBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    ~PinnedBuf() {
        if (p_) (void)hipHostFree(p_);
    }
    int alloc(size_t count) {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        n_ = 0;
        void* q = nullptr;
        HIP_TRY(hipHostMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16, hipHostMallocDefault));
        p_ = static_cast<T*>(q);
        n_ = count;
        return 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    T& operator[](size_t i) const { return p_[i]; }
};

// Engine internals used by the arena (oaz_arena.hip): the search-mode buffers a device-resident fight writes
// its roots to and reads its moves from, and the search of the G roots already in `roots` (enqueued on
// `stream`, the caller being on the engine's device; the moves are then in `moves`).
struct oaz_arena_engine_view {
    int device;
    uint32_t games;
    oaz_state* roots;
    oaz_move* moves;
    hipStream_t stream;
};
int oaz_engine_arena_view(oaz_engine* e, oaz_arena_engine_view* out);
int oaz_engine_search_resident(oaz_engine* e, int G);

// Engine internals used by tree reuse (oaz_tree_reuse.hip: oaz_search_advance, oaz_reuse_stats_get): the trees,
// the resident roots, per-game scratch (allocated with reuse_visits > 0 only: the caller's moves, the
// validation codes, the kept visits), the oaz_reuse_stats counters, and `searched` = the games whose trees are
// the last oaz_search / oaz_search_resume's (0 after self-play). oaz_engine_reuse_advanced records that the
// first G trees now hold at most `most` root visits.
struct oaz_reuse_engine_view {
    int device;
    uint32_t searched, cap;
    int32_t reuse_visits, sims_cap;
    oaz_node* nodes;
    uint32_t* n_nodes;
    oaz_state* roots;
    oaz_move* moves;
    int32_t *codes, *kept;
    uint64_t* counters;
    hipStream_t stream;
    uint64_t seed;  // cfg.seed (oaz_search_sample_moves)
};
int oaz_engine_reuse_view(oaz_engine* e, oaz_reuse_engine_view* out);
int oaz_engine_reuse_advanced(oaz_engine* e, int G, int32_t most);

// Engine internals used by the communicator (oaz_comm.cpp).
int oaz_engine_samples_peek(oaz_engine* e, const oaz_sample** dev, size_t* n, int* device);
int oaz_engine_samples_consume(oaz_engine* e, size_t n);
