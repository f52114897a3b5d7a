// playout_cap_schedule — what csrc/oaz_engine.cpp enqueues for a self-play ply with and without a playout cap, on
// the CPU: engine_schedule.cpp as it is (its fake device, its recording launchers, its log; its own main defined
// away) with recording fakes of the two playout cap launchers and scenarios of its own. Every scenario is printed
// in full. tests/test_playout_cap.py reads the log.
//
// -DPLAYOUT_CAP_OFF_ONLY: only the scenarios without a cap and nothing that names the cap, so that the same file
// also builds against an engine from before the cap; tests/golden/playout_cap_schedule_off.txt was recorded so.
#define main engine_schedule_main
#include "engine_schedule.cpp"
#undef main

#ifndef PLAYOUT_CAP_OFF_ONLY
namespace oaz {
hipError_t launch_playout_cap_masks(const SlotView& v, const CapView& c, hipStream_t s) {
    return launched("playout_cap_masks", s, kn("slots", v.G) + kv("active", v.active) + kv("full", c.full) +
                                                kv("fast", c.fast) + kv("fullm", c.fullm) + kv("nrec", c.nrec) +
                                                kv("cnt", c.cnt) + kn("P", c.P));
}
hipError_t launch_selfplay_move_cap(const TreeView& t, const SlotView& v, const CapView& c, uint32_t temp_plies,
                                    uint64_t* counters, hipStream_t s) {
    return launched("selfplay_move_cap", s, view(t) + kv("root", v.root) + kn("slots", v.G) + kv("full", c.full) +
                                                kv("nrec", c.nrec) + kv("cnt", c.cnt) + kn("temp_plies", temp_plies) +
                                                kv("temp_cnt", counters));
}
}  // namespace oaz
#endif

// 18 simulations (root-noise chunks of 16 + 2), root noise on, one-launch searches allowed (step_kernels 0) and no
// leaf compaction asked for: what a cap-off engine of this size does is its own business, a capped one is forced.
static oaz_config cap_config(int games, int parts) {
    oaz_config c = config(games, 18);
    c.train_noise = 1;
    c.parts = parts;
    return c;
}

// One engine, one self-play ply from a reset; fast > 0: under the cap (fast, share).
static void ply(const char* title, int games, int parts, int fast, int share) {
    begin(title);
    oaz_engine* e = create(cap_config(games, parts));
#ifndef PLAYOUT_CAP_OFF_ONLY
    if (fast) {
        logf("-- set_playout_cap %d %d", fast, share);
        logf("set_playout_cap rc=%d", oaz_selfplay_set_playout_cap(e, fast, share));
    }
#endif
    logf("-- selfplay_step 1");
    logf("selfplay_step rc=%d", oaz_selfplay_step(e, 1));
    report(e, games);
    logf("-- destroy");
    oaz_destroy(e);
}

int main() {
    g_all = true;
    ply("off, 129 games, 1 part", 129, 1, 0, 0);
    ply("off, 2050 games, 2 parts", 2050, 2, 0, 0);
#ifndef PLAYOUT_CAP_OFF_ONLY
    ply("cap 5 of 18, 129 games, 1 part", 129, 1, 5, 16384);
    ply("cap 5 of 18, 2050 games, 2 parts", 2050, 2, 5, 16384);

    begin("refusals");
    {
        oaz_config c = cap_config(129, 1);
        oaz_engine* e = create(c);
        logf("set_playout_cap(18) rc=%d", oaz_selfplay_set_playout_cap(e, 18, 16384));
        logf("selfplay_step rc=%d error=%s", oaz_selfplay_step(e, 1), err_text().c_str());
        logf("set_playout_cap(5) rc=%d", oaz_selfplay_set_playout_cap(e, 5, 16384));
        logf("set_search_time rc=%d", oaz_set_search_time(e, 1000000));
        logf("selfplay_step rc=%d error=%s", oaz_selfplay_step(e, 1), err_text().c_str());
        logf("set_playout_cap(6) rc=%d error=%s", oaz_selfplay_set_playout_cap(e, 6, 16384), err_text().c_str());
        logf("set_playout_cap(0) rc=%d", oaz_selfplay_set_playout_cap(e, 0, 0));
        uint64_t n[2] = {7, 7};
        logf("playout_cap_stats rc=%d full=%llu fast=%llu", oaz_selfplay_playout_cap_stats(e, n), (unsigned long long)n[0],
             (unsigned long long)n[1]);
        oaz_destroy(e);
    }
#endif
    begin("end");
    return 0;
}
