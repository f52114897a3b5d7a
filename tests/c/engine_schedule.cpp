// engine_schedule — records what csrc/oaz_engine.cpp enqueues, on the CPU: the real engine (and oaz_pack.cpp)
// compiled host-only and linked with the fakes below instead of the HIP runtime and the kernels' launchers
// (oaz_kernels.h). No kernel runs; every launch and every HIP call that orders or moves work becomes one log
// line, so "the engine enqueues what it always did" is a text comparison (tests/test_engine_schedule.py,
// tests/golden/engine_schedule.txt). The same idea as rccl_stub.c.
//
// Log notation: sN / eN = the N-th stream / event made in the scenario; aN+B = byte B of the scenario's N-th
// device allocation; "-" = null; "host" = not device memory; "#K" = the K-th launch of the scenario.
// `engine_schedule --full` prints every scenario's device calls; without it all but six are folded into digests.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/onitama_az.h"
#include "../../onitama-alphazero_amd/csrc/oaz_kernels.h"

using namespace oaz;

// ---- the fake device ------------------------------------------------------------------------------
struct Alloc {
    char* base;
    size_t size;
    bool live;
};
static std::vector<Alloc> g_allocs;
static std::vector<bool> g_streams, g_events;  // live flags, by number - 1
static int g_cus = 8;
static long g_launch = 0, g_fail_at = 0;  // launches so far; the launch that fails once (0: none)

// The log. A scenario's device calls (call) are printed, or, in a folded scenario, counted and hashed up to the
// next line of the scenario itself (logf): "(N device calls, fnv1a H)" then stands for them, so the few
// scenarios printed in full keep the log readable and every other one is pinned as tightly by its digests.
static bool g_all = false, g_full = true;  // --full: fold nothing; this scenario is printed in full
static long g_folded = 0;
static uint64_t g_hash = 0;

static void call(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void call(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (n < 0 || n >= (int)sizeof(buf)) abort();
    if (g_full) {
        puts(buf);
        return;
    }
    if (!g_folded++) g_hash = 14695981039346656037ull;
    for (int i = 0; i <= n; ++i) g_hash = (g_hash ^ (unsigned char)buf[i]) * 1099511628211ull;  // the ending 0 too
}

static void logf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void logf(const char* fmt, ...) {
    if (g_folded) printf("(%ld device calls, fnv1a %016llx)\n", g_folded, (unsigned long long)g_hash);
    g_folded = 0;
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    putchar('\n');
}

static std::string ptr(const void* p) {
    if (!p) return "-";
    const char* c = static_cast<const char*>(p);
    for (size_t i = 0; i < g_allocs.size(); ++i)
        if (g_allocs[i].live && c >= g_allocs[i].base && c < g_allocs[i].base + g_allocs[i].size)
            return "a" + std::to_string(i + 1) + "+" + std::to_string((size_t)(c - g_allocs[i].base));
    return "host";
}
static std::string handle(const void* h, const std::vector<bool>& live, char tag) {
    const size_t n = (size_t)(uintptr_t)h;
    if (n == 0) return std::string(1, tag) + "0";
    return std::string(1, tag) + std::to_string(n) + (n <= live.size() && live[n - 1] ? "" : "!dead");
}
static std::string st(hipStream_t s) { return handle(s, g_streams, 's'); }
static std::string ev(hipEvent_t e) { return handle(e, g_events, 'e'); }

extern "C" {
hipError_t hipGetDeviceCount(int* n) { return *n = 1, hipSuccess; }
hipError_t hipGetDevice(int* d) { return *d = 0, hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake launch failure"; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) {
    if (a == hipDeviceAttributeMultiprocessorCount) return *v = g_cus, hipSuccess;
    if (a == hipDeviceAttributeWallClockRate) return *v = 100000, hipSuccess;
    return hipErrorInvalidValue;
}
hipError_t hipMalloc(void** p, size_t n) {
    *p = calloc(n, 1);
    if (!*p) return hipErrorOutOfMemory;
    g_allocs.push_back({static_cast<char*>(*p), n, true});
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    for (Alloc& a : g_allocs)
        if (a.live && a.base == p) {
            a.live = false;
            free(p);
            return hipSuccess;
        }
    return p ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    g_streams.push_back(true);
    *s = (hipStream_t)(uintptr_t)g_streams.size();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { return g_streams[(uintptr_t)s - 1] = false, hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    g_events.push_back(true);
    *e = (hipEvent_t)(uintptr_t)g_events.size();
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { return g_events[(uintptr_t)e - 1] = false, hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { return *ms = 0.5f, hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    call("record %s on %s", ev(e).c_str(), st(s).c_str());
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    call("wait %s for %s", st(s).c_str(), ev(e).c_str());
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    call("sync %s", st(s).c_str());
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t s) {
    call("memcpy %s <- %s %zu %s", ptr(dst).c_str(), ptr(src).c_str(), n, st(s).c_str());
    memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t s) {
    call("memset %s =%d %zu %s", ptr(dst).c_str(), v, n, st(s).c_str());
    memset(dst, v, n);
    return hipSuccess;
}
hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int v, size_t count, hipStream_t s) {
    call("memset32 %s =%d %zu %s", ptr(dst).c_str(), v, count, st(s).c_str());
    for (size_t i = 0; i < count; ++i) static_cast<int*>(dst)[i] = v;
    return hipSuccess;
}
}  // extern "C"

// ---- the fake launchers ---------------------------------------------------------------------------
// One line per launch; the launch numbered g_fail_at fails once.
static hipError_t launched(const char* name, hipStream_t s, const std::string& what) {
    const bool fail = ++g_launch == g_fail_at;
    call("#%ld %s %s%s%s", g_launch, name, st(s).c_str(), what.c_str(), fail ? " -> FAILS" : "");
    return fail ? hipErrorLaunchFailure : hipSuccess;
}
static std::string kv(const char* k, const void* p) { return std::string(" ") + k + "=" + ptr(p); }
static std::string kn(const char* k, long long v) { return std::string(" ") + k + "=" + std::to_string(v); }
// the games of the view (n_nodes is [G]: its offset / 4 is the first game), its bucket counters, compaction or not
static std::string view(const TreeView& t) {
    return kn("G", t.G) + kv("games", t.n_nodes) + kv("bcnt", t.bcnt) + kn("need", t.need != nullptr) +
           kn("slot", t.slot != nullptr);
}
static std::string nn(const NNView* w) {
    if (!w) return " nn=-";
    return kn("precision", w->precision) + kn("small_max", w->small_max) + kv("tm.bcnt", w->tm.bcnt) +
           kn("tm.nb", w->tm.nb) + kn("tm.cap", w->tm.cap);
}

namespace oaz {
bool tree_seg_kernels() { return true; }
hipError_t launch_movegen(const oaz_state*, int n, uint32_t*, oaz_move*, uint8_t*, hipStream_t s) {
    return launched("movegen", s, kn("n", n));
}
hipError_t launch_step(oaz_state*, const oaz_move*, int n, uint8_t*, hipStream_t s) { return launched("step", s, kn("n", n)); }
hipError_t launch_current_state(const oaz_state*, int n, uint8_t*, hipStream_t s) {
    return launched("current_state", s, kn("n", n));
}
hipError_t launch_encode(const oaz_state*, int n, float*, hipStream_t s) { return launched("encode", s, kn("n", n)); }
hipError_t launch_nn_forward(const NNView& w, const oaz_state* s, int B, float* policy, float* value, hipStream_t q) {
    return launched("nn_forward", q, kn("B", B) + kv("states", s) + kv("policy", policy) + kv("value", value) + nn(&w));
}
hipError_t launch_hash_eval(const oaz_state* s, int B, float* policy, float* value, hipStream_t q) {
    return launched("hash_eval", q, kn("B", B) + kv("states", s) + kv("policy", policy) + kv("value", value));
}
hipError_t launch_eval_compact(const TreeView& t, hipStream_t s) { return launched("eval_compact", s, view(t)); }
hipError_t launch_tree_reset(const TreeView& t, hipStream_t s) { return launched("tree_reset", s, view(t)); }
hipError_t launch_select(const TreeView& t, const oaz_state* roots, const uint8_t* active, const noise_t* noise,
                         SearchParams, hipStream_t s) {
    return launched("select", s, view(t) + kv("roots", roots) + kv("active", active) + kv("noise", noise));
}
hipError_t launch_root_noise(const oaz_state* roots, const uint8_t* active, const uint64_t* game_id, const uint32_t* ply,
                             SearchParams, uint32_t G, uint32_t sim0, uint32_t nsims, noise_t* out, hipStream_t s) {
    return launched("root_noise", s, kn("G", G) + kn("sim0", sim0) + kn("nsims", nsims) + kv("roots", roots) +
                                         kv("active", active) + kv("game_id", game_id) + kv("ply", ply) + kv("out", out));
}
hipError_t launch_expand_backup(const TreeView& t, const oaz_state* roots, const uint8_t* active, const float* policy,
                                const float* value, hipStream_t s) {
    return launched("expand_backup", s,
                    view(t) + kv("roots", roots) + kv("active", active) + kv("policy", policy) + kv("value", value));
}
hipError_t launch_backup_select(const TreeView& t, const oaz_state* roots, const uint8_t* active, const float* policy,
                                const float* value, const noise_t* noise, SearchParams, hipStream_t s) {
    return launched("backup_select", s, view(t) + kv("roots", roots) + kv("active", active) + kv("policy", policy) +
                                            kv("value", value) + kv("noise", noise));
}
hipError_t launch_search_finalize(const TreeView& t, const oaz_state* roots, oaz_move* out_move, float* out_pi,
                                  hipStream_t s) {
    return launched("search_finalize", s, view(t) + kv("roots", roots) + kv("move", out_move) + kv("pi", out_pi));
}
// The two one-launch searches also leave what the kernels would without a deadline: every game ran them all.
hipError_t launch_search_lat(const TreeView& t, const oaz_state* roots, const uint8_t* active, SearchParams, int sims,
                             const NNView* w, float* policy, float* value, const uint64_t* deadline, uint32_t* sims_run,
                             hipStream_t s) {
    const hipError_t rc = launched("search_lat", s, view(t) + kn("sims", sims) + kv("roots", roots) + kv("active", active) +
                                                        kv("policy", policy) + kv("value", value) + kv("deadline", deadline) +
                                                        kv("sims_run", sims_run) + nn(w));
    for (uint32_t g = 0; sims_run && rc == hipSuccess && g < t.G; ++g) sims_run[g] = (uint32_t)sims;
    return rc;
}
hipError_t launch_search_grp(const TreeView& t, const oaz_state* roots, const uint8_t* active, SearchParams, int s0, int s1,
                             const noise_t* noise, const NNView* w, float* policy, float* value, const uint64_t* deadline,
                             uint32_t* sims_run, hipStream_t s) {
    const hipError_t rc =
        launched("search_grp", s, view(t) + kn("s0", s0) + kn("s1", s1) + kv("roots", roots) + kv("active", active) +
                                      kv("noise", noise) + kv("policy", policy) + kv("value", value) +
                                      kv("deadline", deadline) + kv("sims_run", sims_run) + nn(w));
    for (uint32_t g = 0; sims_run && rc == hipSuccess && g < t.G; ++g) sims_run[g] = (uint32_t)s1;
    return rc;
}
hipError_t launch_deadline_start(uint64_t* deadline, uint64_t ticks, hipStream_t s) {
    return launched("deadline_start", s, kv("deadline", deadline) + kn("ticks", (long long)ticks));
}
hipError_t launch_selfplay_move(const TreeView& t, const SlotView& v, hipStream_t s) {
    return launched("selfplay_move", s, view(t) + kv("root", v.root) + kn("slots", v.G));
}
hipError_t launch_selfplay_reset(const TreeView& t, const SlotView& v, hipStream_t s) {
    return launched("selfplay_reset", s, view(t) + kv("root", v.root) + kn("slots", v.G));
}
hipError_t launch_stats_reduce(const uint64_t* per_game, uint32_t G, uint64_t* out, hipStream_t s) {
    return launched("stats_reduce", s, kn("G", G) + kv("stats", per_game) + kv("out", out));
}
}  // namespace oaz

// ---- scenarios --------------------------------------------------------------------------------------
// The error text without HIP_TRY's trailing " (file:line)", which names the build's path and the source line.
static std::string err_text() {
    std::string s = oaz_last_error();
    const size_t p = s.rfind(" (");
    if (p != std::string::npos && !s.empty() && s.back() == ')') s.erase(p);
    return s;
}

static void begin(const char* title) {
    size_t live = 0;
    for (const Alloc& a : g_allocs) live += a.live;
    for (bool b : g_streams) live += b;
    for (bool b : g_events) live += b;
    if (live) logf("LEAKED %zu device resources before this scenario", live);
    g_allocs.clear();
    g_streams.clear();
    g_events.clear();
    g_launch = g_fail_at = 0;
    logf("==== %s", title);
    // printed in full: one scenario of each path and kind
    static const char* const full[] = {"1 lat, budget 1e9", "2 grp, one chunk", "4 steps, small, compact 0, timing 0",
                                       "5 steps, NN, 2048 games (2 parts)", "8 self-play, 6 games, 2 parts, 3 sims, root noise",
                                       "10 a part-1 launch in the middle of a step fails"};
    g_full = g_all;
    for (const char* f : full) g_full = g_full || !strcmp(f, title);
}

// HASH evaluator, no root noise, tiny self-play buffers: only the search's own sizes matter here.
static oaz_config config(int games, int sims) {
    oaz_config c;
    oaz_config_default(&c);
    c.blocks = 2;
    c.games = games;
    c.sims = sims;
    c.evaluator = OAZ_EVAL_HASH;
    c.train_noise = 0;
    c.max_plies = 2;
    c.sample_capacity = 16;
    c.fixed_deck = 1;
    return c;
}

static oaz_engine* create(const oaz_config& c, int timing = 0) {
    logf("-- create games=%d sims=%d evaluator=%d noise=%d compact=%d parts=%d step_kernels=%d search_time_ns=%lld timing=%d",
         c.games, c.sims, c.evaluator, c.train_noise, c.compact, c.parts, c.step_kernels, (long long)c.search_time_ns, timing);
    oaz_engine* e = oaz_create(&c, 0);
    if (!e) {
        logf("create failed: %s", err_text().c_str());
        exit(1);
    }
    if (timing) logf("set_timing rc=%d", oaz_set_timing(e, timing));
    return e;
}

static void report(oaz_engine* e, int G) {
    logf("-- report");
    oaz_kernel_times k;
    int rc = oaz_kernel_times_get(e, &k);
    logf("kernel_times rc=%d select=%llu nn=%llu expand=%llu finalize=%llu noise=%llu compact=%llu backup_select=%llu "
         "nn_samples=%llu nn_busy=%llu parts=%llu", rc, (unsigned long long)k.select_n, (unsigned long long)k.nn_n,
         (unsigned long long)k.expand_n, (unsigned long long)k.finalize_n, (unsigned long long)k.noise_n,
         (unsigned long long)k.compact_n, (unsigned long long)k.backup_select_n, (unsigned long long)k.nn_samples,
         (unsigned long long)k.nn_busy_n, (unsigned long long)k.parts);
    logf("kernel_ms select=%.1f nn=%.1f expand=%.1f finalize=%.1f noise=%.1f compact=%.1f backup_select=%.1f nn_busy=%.1f",
         k.select_ms, k.nn_ms, k.expand_ms, k.finalize_ms, k.noise_ms, k.compact_ms, k.backup_select_ms, k.nn_busy_ms);
    int last = -1;
    rc = oaz_last_sims(e, &last);
    logf("last_sims rc=%d sims=%d", rc, last);
    std::vector<int> n((size_t)G, -1);
    rc = oaz_search_playouts(e, n.data(), G);
    int lo = n.empty() ? 0 : n[0], hi = lo;
    for (int v : n) lo = v < lo ? v : lo, hi = v > hi ? v : hi;
    logf("search_playouts rc=%d games=%d min=%d max=%d", rc, G, lo, hi);
}

static int search(oaz_engine* e, int G) {
    logf("-- search G=%d", G);
    uint8_t deck[5] = {0, 1, 2, 3, 4};
    std::vector<oaz_state> roots((size_t)G);
    for (oaz_state& r : roots) oaz_initial_state(deck, &r);
    std::vector<oaz_move> mv((size_t)G);
    std::vector<float> pi((size_t)G * 50);
    const int rc = oaz_search(e, roots.data(), G, mv.data(), pi.data(), nullptr, nullptr);
    logf("search rc=%d%s%s", rc, rc ? " error=" : "", rc ? err_text().c_str() : "");
    return rc;
}

// One engine, one search of all its games (or of G of them), the report, destroy.
static void run(const char* title, const oaz_config& c, int timing = 0, int G = 0) {
    begin(title);
    oaz_engine* e = create(c, timing);
    if (!G) G = c.games;
    search(e, G);
    report(e, G);
    logf("-- destroy");
    oaz_destroy(e);
}

// The per-step loop at its smallest: 5 games in 2 parts (4 asked for), chunks of 16 + 2 simulations, root noise.
static oaz_config steps_small() {
    oaz_config c = config(5, 18);
    c.step_kernels = 1;
    c.parts = 4;
    c.train_noise = 1;
    return c;
}

static void run_failing(const char* title, long k) {
    begin(title);
    oaz_engine* e = create(steps_small());
    g_fail_at = k;
    search(e, 5);
    logf("-- after the failed search");
    const int rc = oaz_sync(e);
    logf("sync rc=%d last_error=%s", rc, err_text().c_str());
    oaz_destroy(e);
    logf("destroyed last_error=%s", err_text().c_str());
}

int main(int argc, char** argv) {
    g_all = argc > 1 && !strcmp(argv[1], "--full");  // every scenario in full: to diff two engines' schedules
    // scenario 10's failing launches, read off scenario 4's log (compact 0, timing 0): #3 the second root_noise
    // (after the parts' fork), #30 part 1's backup_select of simulation 6, #77 the last expand_backup
    const long fail[3] = {3, 30, 77};
    oaz_config c;

    // 1. k_search_lat
    c = config(3, 7);
    run("1 lat", c);
    c.search_time_ns = 1000000000;
    run("1 lat, budget 1e9", c);
    run("1 lat, budget 1e9, timing 1", c, 1);
    c.search_time_ns = 0;
    run("1 lat, timing 1", c, 1);

    // 2. k_search_grp, one chunk (root noise excludes lat)
    c = config(3, 40);
    c.train_noise = 1;
    run("2 grp, one chunk", c);
    run("2 grp, one chunk, timing 1", c, 1);

    // 3. k_search_grp, three chunks, at the last G that qualifies (16 games x 8 CUs) and the first that does not
    c = config(128, 1100);
    c.train_noise = 1;
    run("3 grp, three chunks, 128 games", c);
    c.search_time_ns = 1000000000;
    run("3 grp, three chunks, 128 games, budget 1e9", c);
    c = config(129, 1100);
    c.train_noise = 1;
    run("3 129 games: the per-step loop", c);

    // 4. the per-step loop, small
    for (int compact = 0; compact < 2; ++compact)
        for (int timing = 0; timing < 4; timing += 3) {
            c = steps_small();
            c.compact = compact;
            const std::string title = "4 steps, small, compact " + std::to_string(compact) + ", timing " + std::to_string(timing);
            run(title.c_str(), c, timing);
        }

    // 5. the per-step loop, the network, automatic parts
    c = config(2047, 3);
    c.evaluator = OAZ_EVAL_NN;
    c.precision = OAZ_FP32_SPLIT16;
    c.compact = 1;
    run("5 steps, NN, 2047 games (1 part)", c);
    c.games = 2048;
    run("5 steps, NN, 2048 games (2 parts)", c);
    c.games = 8200;
    c.sims = 2;
    c.parts = 4;
    run("5 steps, NN, 8200 games, 4 parts (3 buckets)", c);

    // 6. compact = 2: from 12 x 16 x CUs games
    c = config(1535, 2);
    c.compact = 2;
    run("6 compact 2, 1535 games", c);
    c.games = 1536;
    run("6 compact 2, 1536 games", c);

    // 7. the host budget on the per-step loop: never spent, and spent after the first step
    c = steps_small();
    c.search_time_ns = 1000000000;
    run("7 steps, small, budget 1e9", c);
    c.search_time_ns = 1;
    run("7 steps, small, budget 1 ns", c);

    // 8. self-play
    begin("8 self-play, 6 games, 2 parts, 3 sims, root noise");
    c = config(6, 3);
    c.step_kernels = 1;
    c.parts = 2;
    c.train_noise = 1;
    {
        oaz_engine* e = create(c);
        logf("-- selfplay_reset");
        logf("selfplay_reset rc=%d", oaz_selfplay_reset(e));
        logf("-- selfplay_step 2");
        logf("selfplay_step rc=%d", oaz_selfplay_step(e, 2));
        report(e, 6);
        logf("-- destroy");
        oaz_destroy(e);
    }

    // 9. a few roots on a large engine
    c = config(2048, 18);
    run("9 5 roots of 2048 games", c, 0, 5);
    c.train_noise = 1;
    run("9 5 roots of 2048 games, root noise", c, 0, 5);

    // 10. a failing launch (of the fake: nothing here touches a device)
    run_failing("10 a root_noise launch fails", fail[0]);
    run_failing("10 a part-1 launch in the middle of a step fails", fail[1]);
    run_failing("10 the last expand_backup fails", fail[2]);
    begin("end");
    return 0;
}
