/* arena_smoke.c — oaz_arena_fight from plain C against include/onitama_az.h alone: a HASH-evaluator engine
 * against the Random agent, 6 games, twice: the second fight after oaz_destroy and a fresh oaz_create, so the
 * fight's use of the engine's buffers is covered across an engine's lifetime. Prints one line per fight:
 *   fight <i> rc <rc> results r0..r5 plies p0..p5 wld <w> <l> <d> passes <n> total <n> ratings <a> <b>
 * usage: arena_smoke <sims> <max_plies> <deal_seed> <random_seed> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "onitama_az.h"

enum { GAMES = 6 };

static int one_fight(int i, int sims, int max_plies, unsigned long long deal_seed, unsigned long long random_seed) {
    oaz_arena_config ac;
    oaz_arena_config_default(&ac);
    ac.game_amnt = GAMES;
    ac.max_plies = max_plies;
    ac.seed = deal_seed;
    int32_t need[2];
    if (oaz_arena_capacity(&ac, need) != OAZ_OK) {
        fprintf(stderr, "capacity: %s\n", oaz_last_error());
        return 1;
    }
    oaz_config cfg;
    oaz_config_default(&cfg);
    cfg.blocks = 0;
    cfg.evaluator = OAZ_EVAL_HASH;
    cfg.sims = sims;
    cfg.c_puct = 1.4142135623730951;
    cfg.train_noise = 0;
    cfg.games = need[0];
    oaz_engine* eng = oaz_create(&cfg, 0);
    if (!eng) {
        fprintf(stderr, "create: %s\n", oaz_last_error());
        return 1;
    }
    oaz_arena_agent agent, opponent;
    memset(&agent, 0, sizeof(agent));
    memset(&opponent, 0, sizeof(opponent));
    agent.kind = OAZ_AGENT_ALPHAZERO;
    agent.engine = eng;
    opponent.kind = OAZ_AGENT_RANDOM;
    opponent.seed = random_seed;
    oaz_fight_stats st;
    uint8_t results[GAMES];
    int32_t plies[GAMES];
    double history[GAMES * 4];
    const int rc = oaz_arena_fight(&ac, &agent, &opponent, 800.0, 800.0, &st, results, plies, history);
    oaz_destroy(eng);
    if (rc != OAZ_OK) {
        fprintf(stderr, "fight: %s\n", oaz_last_error());
        return 1;
    }
    printf("fight %d rc %d results", i, rc);
    for (int k = 0; k < GAMES; ++k) printf(" %d", results[k]);
    printf(" plies");
    for (int k = 0; k < GAMES; ++k) printf(" %d", plies[k]);
    printf(" wld %u %u %u passes %llu total %llu ratings %.17g %.17g\n", st.wins, st.loses, st.draws,
           (unsigned long long)st.passes, (unsigned long long)st.plies_total, st.rating_a, st.rating_b);
    if (history[0] != 800.0 || history[4 * (GAMES - 1) + 1] != st.rating_a) {
        fprintf(stderr, "history does not start at the given rating or end at the final one\n");
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: arena_smoke <sims> <max_plies> <deal_seed> <random_seed>\n");
        return 2;
    }
    if (oaz_abi_version() != OAZ_ABI_VERSION) return 3;
    const int sims = atoi(argv[1]), max_plies = atoi(argv[2]);
    const unsigned long long deal_seed = strtoull(argv[3], NULL, 10), random_seed = strtoull(argv[4], NULL, 10);
    for (int i = 0; i < 2; ++i)
        if (one_fight(i, sims, max_plies, deal_seed, random_seed + (unsigned)i)) return 1;
    return 0;
}
