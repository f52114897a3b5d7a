// oaz_device.h — rules, RNG and evaluator primitives shared by the HIP kernels and the host
// engine (all __host__ __device__). Semantics follow the reference exactly (citations per
// function); the formulation is the GPU's own (branch-free bit ops, one lane per square).
#pragma once

#include <stdint.h>

#include "../../include/onitama_az.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OAZ_HD __host__ __device__ __forceinline__
#else
#define OAZ_HD inline
#endif

namespace oaz {

// ---- cards: onitama-game/src/game/card.rs:17-468 -------------------------------------
// Card patterns are 25-bit masks (bit 31-i = square i) centred on square 12; `mirror` is
// the pattern Blue uses (card.rs:531-533).
constexpr uint32_t kCardPos[16] = {0x20004000u, 0x0440A000u, 0x02202000u, 0x00828000u,
                                   0x01220000u, 0x02940000u, 0x02142000u, 0x00948000u,
                                   0x0280A000u, 0x02804000u, 0x0100A000u, 0x01104000u,
                                   0x01044000u, 0x01140000u, 0x02048000u, 0x00902000u};
constexpr uint32_t kCardMir[16] = {0x01000200u, 0x02811000u, 0x02022000u, 0x00A08000u,
                                   0x00224000u, 0x0014A000u, 0x02142000u, 0x00948000u,
                                   0x0280A000u, 0x0100A000u, 0x02804000u, 0x01044000u,
                                   0x01104000u, 0x00144000u, 0x00902000u, 0x02048000u};
// Card.player_color (0 Red, 1 Blue): the first mover is the neutral card's colour.
constexpr uint8_t kCardColor[16] = {1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0};

constexpr uint32_t kRedKingStart = 0x00000200u;   // state.rs:24
constexpr uint32_t kBlueKingStart = 0x20000000u;  // state.rs:31
constexpr uint32_t kBluePawnsStart = 0xD8000000u; // state.rs:38
constexpr uint32_t kRedPawnsStart = 0x00000D80u;  // state.rs:45
constexpr int kBlueTemple = 2;                    // state.rs:48
constexpr int kRedTemple = 22;                    // state.rs:49

OAZ_HD constexpr uint32_t sq_bit(int sq) { return 0x80000000u >> sq; }

// ATTACK_MAPS[color][card][from] (card.rs:476-604). The reference builds it by shifting the
// centred pattern by the square delta and masking wrapped files by (delta % 5). Here every
// pattern square is turned into a (dr, dc) offset from the centre and applied to `from`
// when it stays on the board — the same set (the file masks remove exactly the column
// wrap-arounds; tests/test_host.py::test_attack_maps_equal_oracle checks the tables against the oracle).
struct AttackTable {
    uint32_t m[2][16][25];
};

constexpr AttackTable make_attack_table() {
    AttackTable t{};
    for (int color = 0; color < 2; ++color)
        for (int card = 0; card < 16; ++card) {
            const uint32_t pat = color ? kCardMir[card] : kCardPos[card];
            for (int from = 0; from < 25; ++from) {
                uint32_t m = 0;
                for (int j = 0; j < 25; ++j) {
                    if (!(pat & sq_bit(j))) continue;
                    const int dr = j / 5 - 2, dc = j % 5 - 2;
                    const int r = from / 5 + dr, c = from % 5 + dc;
                    if (r >= 0 && r < 5 && c >= 0 && c < 5) m |= sq_bit(r * 5 + c);
                }
                t.m[color][card][from] = m;
            }
        }
    return t;
}

constexpr AttackTable kAttackHost = make_attack_table();

// ---- state helpers ----------------------------------------------------------------------
OAZ_HD bool is_win(int r) { return r == OAZ_RED_WIN || r == OAZ_BLUE_WIN; }

// State::make_move (state.rs:145-202) + Deck::rotate (deck.rs:87-90); colour = mover.
OAZ_HD int make_move(oaz_state& s, int from, int to, int piece, int slot, int color) {
    const uint32_t fb = sq_bit(from), tb = sq_bit(to);
    const int enemy = color ^ 1;
    if (piece == OAZ_PAWN) s.pawns[color] &= ~fb;
    else s.kings[color] &= ~fb;
    int res = OAZ_IN_PROGRESS;
    if (s.pawns[enemy] & tb) {
        s.pawns[enemy] &= ~tb;
        res = OAZ_CAPTURE;
    } else if (s.kings[enemy] & tb) {
        s.kings[enemy] &= ~tb;
        res = color == OAZ_RED ? OAZ_RED_WIN : OAZ_BLUE_WIN;
    }
    if (piece == OAZ_PAWN) s.pawns[color] |= tb;
    else s.kings[color] |= tb;
    if (piece == OAZ_KING && to == (color == OAZ_RED ? kBlueTemple : kRedTemple))
        res = color == OAZ_RED ? OAZ_RED_WIN : OAZ_BLUE_WIN;
    if (slot < 4) {
        const uint8_t t = s.cards[slot];
        s.cards[slot] = s.cards[4];
        s.cards[4] = t;
    }
    return res;
}

// Register-only forms of the colour- and slot-indexed accesses, for code that holds the state in registers
// across a loop (the one-launch search's walk): a runtime index into the struct (s.pawns[color],
// s.cards[slot]) can make the compiler keep the whole state in scratch memory, a memory round trip per
// access. cards[0..3] are one little-endian word.
OAZ_HD int state_card(const oaz_state& s, int i) {
    uint32_t w;
    __builtin_memcpy(&w, s.cards, 4);
    return i < 4 ? (int)((w >> (8 * i)) & 0xFFu) : (int)s.cards[4];
}
OAZ_HD void state_rotate(oaz_state& s, int slot) {  // Deck::rotate (deck.rs:87-90): cards[slot] <-> cards[4]
    uint32_t w;
    __builtin_memcpy(&w, s.cards, 4);
    const uint32_t sh = 8u * (uint32_t)slot;
    const uint8_t t = (uint8_t)(w >> sh);
    w = (w & ~(0xFFu << sh)) | ((uint32_t)s.cards[4] << sh);
    __builtin_memcpy(s.cards, &w, 4);
    s.cards[4] = t;
}
// make_move with the same result and state, through selects
OAZ_HD int make_move_regs(oaz_state& s, int from, int to, int piece, int slot, int color) {
    const uint32_t fb = sq_bit(from), tb = sq_bit(to);
    const bool blue = color != OAZ_RED;
    uint32_t mp = blue ? s.pawns[1] : s.pawns[0], mk = blue ? s.kings[1] : s.kings[0];
    uint32_t ep = blue ? s.pawns[0] : s.pawns[1], ek = blue ? s.kings[0] : s.kings[1];
    if (piece == OAZ_PAWN) mp &= ~fb;
    else mk &= ~fb;
    int res = OAZ_IN_PROGRESS;
    if (ep & tb) {
        ep &= ~tb;
        res = OAZ_CAPTURE;
    } else if (ek & tb) {
        ek &= ~tb;
        res = color == OAZ_RED ? OAZ_RED_WIN : OAZ_BLUE_WIN;
    }
    if (piece == OAZ_PAWN) mp |= tb;
    else mk |= tb;
    if (piece == OAZ_KING && to == (color == OAZ_RED ? kBlueTemple : kRedTemple))
        res = color == OAZ_RED ? OAZ_RED_WIN : OAZ_BLUE_WIN;
    s.pawns[0] = blue ? ep : mp;
    s.pawns[1] = blue ? mp : ep;
    s.kings[0] = blue ? ek : mk;
    s.kings[1] = blue ? mk : ek;
    if (slot < 4) state_rotate(s, slot);
    return res;
}

// State::current_state (state.rs:120-134)
OAZ_HD int current_state(const oaz_state& s) {
    if (s.kings[0] == 0 || s.kings[1] == kRedKingStart) return OAZ_BLUE_WIN;
    if (s.kings[1] == 0 || s.kings[0] == kBlueKingStart) return OAZ_RED_WIN;
    return OAZ_IN_PROGRESS;
}

// reward (alphazero_mcts/mod.rs:45-53)
OAZ_HD double reward(int result, int color) {
    if (!is_win(result)) return 0.0;
    return ((result == OAZ_RED_WIN) == (color == OAZ_RED)) ? 1.0 : -1.0;
}

// State::with_deck (state.rs:66-72); first mover = neutral card colour (game_state.rs:37-45)
OAZ_HD void initial_state(const uint8_t deck[5], oaz_state& s) {
    s.kings[0] = kRedKingStart;
    s.kings[1] = kBlueKingStart;
    s.pawns[0] = kRedPawnsStart;
    s.pawns[1] = kBluePawnsStart;
    for (int i = 0; i < 5; ++i) s.cards[i] = deck[i];
    s.to_move = kCardColor[deck[4] & 15];
    s.pad[0] = s.pad[1] = 0;
}

// Packed move (oaz_node.mv): from | to<<5 | slot<<10 | piece<<12
OAZ_HD uint16_t pack_move(int from, int to, int slot, int piece) {
    return (uint16_t)(from | (to << 5) | (slot << 10) | (piece << 12));
}
OAZ_HD int mv_from(uint32_t m) { return m & 31; }
OAZ_HD int mv_to(uint32_t m) { return (m >> 5) & 31; }
OAZ_HD int mv_slot(uint32_t m) { return (m >> 10) & 3; }
OAZ_HD int mv_piece(uint32_t m) { return (m >> 12) & 1; }

// ---- counter-based RNG (DESIGN.md "RNG"): Philox4x32-10 ---------------------------------
struct u32x4 {
    uint32_t x, y, z, w;
};

OAZ_HD u32x4 philox(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// uniform in (0,1) with 53 random bits
OAZ_HD double u01(uint32_t a, uint32_t b) {
    const uint64_t m = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
    return ((double)m + 0.5) * (1.0 / 9007199254740992.0);
}

// ---- Dirichlet root noise (mcts_arena.rs:186-203) ------------------------------------------
// The reference draws a fresh Dirichlet(alpha; K) vector (f64, rand_distr 0.4.3: gamma variates,
// Marsaglia-Tsang with the u^(1/shape) boost for shape < 1, normalised) for every PUCT evaluation at
// the root and uses component child.idx-1: marginally Beta(alpha, (K-1) alpha) = X / (X + Y) with
// X ~ Gamma(alpha), Y ~ Gamma((K-1) alpha). The noise parity with the reference is distributional (its
// thread_rng is unseedable); the draw here is the same Beta marginal in f64, by Johnk's method in the log
// domain (U^(1/0.03) underflows even in f64 for U < 1e-9). log and exp are the polynomials below: only
// IEEE +, -, *, / and explicit fused multiply-adds (correctly rounded on the host, x86 vfmadd / libm fma,
// and on the device, v_fma_f64) with no compiler contraction, so the device, the host (oaz_root_noise)
// and the C oracle compute bit-identical draws.
// (The f32 draw this replaced is gone; its A/B is profiles/r06b_noise_f64_vs_f32_ab.log.)
typedef double noise_t;  // one draw, as the engine's noise ring stores it

// ln 2 split: kLn2Hi has 21 trailing zero bits (k * kLn2Hi is exact for |k| < 2^21), kLn2Lo the rest.
constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10;
OAZ_HD double nz_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// natural log for normal x > 0: x = 2^e m, m in [sqrt(1/2), sqrt(2)), t = (m - 1) / (m + 1), log m =
// 2 atanh(t) = 2 (t + t^3 / 3 + ... + t^21 / 21) (|t| <= 0.1716: the next term is < 1e-18 relative).
OAZ_HD double nz_log64(double x) {
    uint64_t b = __builtin_bit_cast(uint64_t, x);
    int e = (int)((b >> 52) & 0x7FF) - 1023;
    double m = __builtin_bit_cast(double, (b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e += 1;
    }
    const double t = (m - 1.0) / (m + 1.0), t2 = t * t;
    double p = 2.0 / 21.0;
    p = nz_fma(p, t2, 2.0 / 19.0);
    p = nz_fma(p, t2, 2.0 / 17.0);
    p = nz_fma(p, t2, 2.0 / 15.0);
    p = nz_fma(p, t2, 2.0 / 13.0);
    p = nz_fma(p, t2, 2.0 / 11.0);
    p = nz_fma(p, t2, 2.0 / 9.0);
    p = nz_fma(p, t2, 2.0 / 7.0);
    p = nz_fma(p, t2, 2.0 / 5.0);
    p = nz_fma(p, t2, 2.0 / 3.0);
    p = nz_fma(p * t2, t, 2.0 * t);  // t (2 + t2 p)
    const double de = (double)e;
    return nz_fma(de, kLn2Hi, nz_fma(de, kLn2Lo, p));
}
// e^x: x = k ln2 + r, |r| <= ln2 / 2, Taylor to r^13 (the remainder is < 5e-18 relative); 0 below -708
// (the normal range), +inf above 709.
OAZ_HD double nz_exp64(double x) {
    if (x < -708.0) return 0.0;
    if (x > 709.0) return __builtin_bit_cast(double, 0x7FF0000000000000ull);
    const double k = (double)(int)(x * 1.4426950408889634 + (x >= 0.0 ? 0.5 : -0.5));
    const double r = (x - k * kLn2Hi) - k * kLn2Lo;
    double q = 1.0 / 6227020800.0;  // 1 / 13!
    q = nz_fma(q, r, 1.0 / 479001600.0);
    q = nz_fma(q, r, 1.0 / 39916800.0);
    q = nz_fma(q, r, 1.0 / 3628800.0);
    q = nz_fma(q, r, 1.0 / 362880.0);
    q = nz_fma(q, r, 1.0 / 40320.0);
    q = nz_fma(q, r, 1.0 / 5040.0);
    q = nz_fma(q, r, 1.0 / 720.0);
    q = nz_fma(q, r, 1.0 / 120.0);
    q = nz_fma(q, r, 1.0 / 24.0);
    q = nz_fma(q, r, 1.0 / 6.0);
    q = nz_fma(q, r, 0.5);
    q = nz_fma(q, r, 1.0);
    q = nz_fma(q, r, 1.0);
    return q * __builtin_bit_cast(double, (uint64_t)((int64_t)k + 1023) << 52);
}
// Draw idx (2j + {0: running best, 1: child j}) of comparison j; c2 = ply << 16 | sim.
// Beta(a, b), a = alpha, b = (K - 1) alpha, by Johnk's method: with U, V uniform, X = U^(1/a),
// Y = V^(1/b), the pairs with X + Y <= 1 give X / (X + Y) ~ Beta(a, b) exactly (acceptance
// Gamma(a+1) Gamma(b+1) / Gamma(a+b+1): 0.99 at K = 12, 0.96 at K = 40). In the log domain:
// lx = log(U) / a, ly = log(V) / b (as products with the rounded reciprocals), X = exp(lx), Y = exp(ly),
// accept when X + Y <= 1, eta = X / (X + Y) when both are normal, else (one of them below e^-708) in the
// log domain, eta = 1 / (1 + exp(ly - lx)). Attempt t takes Philox block (game lo, game hi, c2,
// idx << 12 | t): U from words 0, 1 and V from words 2, 3 (53-bit uniforms, u01).
// Resolution: eta is 1.0 exactly when Y / X < 2^-53, as the reference's X / (X + Y) in f64 is.
OAZ_HD double root_noise_f64(uint64_t seed, uint64_t game, uint32_t c2, uint32_t idx, double alpha, int K) {
    const double ia = 1.0 / alpha, ib = 1.0 / (alpha * (double)(K - 1));
    for (uint32_t t = 0; t < 2048u; ++t) {
        const u32x4 r = philox(seed, (uint32_t)game, (uint32_t)(game >> 32), c2, (idx << 12) | t);
        const double lx = nz_log64(u01(r.x, r.y)) * ia, ly = nz_log64(u01(r.z, r.w)) * ib;
        const double x = nz_exp64(lx), y = nz_exp64(ly), sum = x + y;
        if (sum <= 1.0) return (x > 0.0 && y > 0.0) ? x / sum : 1.0 / (1.0 + nz_exp64(ly - lx));
    }
    return 1.0 / (double)K;  // (never reached: 2048 rejections in a row)
}
// The engine's draw (k_root_noise, oaz_root_noise).
OAZ_HD noise_t root_noise(uint64_t seed, uint64_t game, uint32_t c2, uint32_t idx, double alpha, int K) {
    return root_noise_f64(seed, game, c2, idx, alpha, K);
}

// Deck::default (deck.rs:139-151): random 5 of the 16 cards; Fisher-Yates driven by
// Philox(seed; game_id, 0xDEA1, q).
OAZ_HD void deal_deck(uint64_t seed, uint64_t game_id, uint8_t out[5]) {
    uint8_t cards[16];
    for (int i = 0; i < 16; ++i) cards[i] = (uint8_t)i;
    uint32_t w[16];
    for (uint32_t q = 0; q < 4; ++q) {
        const u32x4 r = philox(seed, (uint32_t)game_id, (uint32_t)(game_id >> 32), 0xDEA1u, q);
        w[4 * q] = r.x;
        w[4 * q + 1] = r.y;
        w[4 * q + 2] = r.z;
        w[4 * q + 3] = r.w;
    }
    for (int i = 15, k = 0; i >= 1; --i, ++k) {
        const uint32_t j = (uint32_t)(((uint64_t)w[k] * (uint64_t)(i + 1)) >> 32);
        const uint8_t t = cards[i];
        cards[i] = cards[j];
        cards[j] = t;
    }
    for (int i = 0; i < 5; ++i) out[i] = cards[i];
}

// Global game id of self-play slot g of rank r (of `world` ranks, G slots each) in the slot's seq-th
// game: (seq * world + r) * G + g. The id keys the deal and the root noise, so
// ranks play disjoint games and together every id below (seq + 1) * world * G once per sequence;
// k_selfplay_move's start_game and the host's oaz_slot_game_ids both call this.
OAZ_HD uint64_t slot_game_id(uint64_t seq, uint32_t world, uint32_t rank, uint32_t G, uint32_t g) {
    return (seq * (uint64_t)world + (uint64_t)rank) * (uint64_t)G + (uint64_t)g;
}

// ---- self-play temperature (oaz_config.temperature_plies; DESIGN.md "Self-play temperature") -------------
// In the first T plies of a self-play game the played move is drawn in proportion to the root children's visits
// (tau = 1), in integers: with S = the sum of the visits n_0 .. n_{K-1} (uint32) and w = word 0 of
// Philox(seed; game lo, game hi, 0x54454D50 "TEMP", ply), r = (w * S) >> 32 is uniform on [0, S) and the played
// child is the first j whose inclusive prefix sum n_0 + .. + n_j exceeds r: child j with probability n_j / S up
// to 2^-32 S, a child without visits never. The tag is >= 2^24, so no root-noise word (ply << 16 | sim) equals it.
constexpr uint32_t kTemperatureTag = 0x54454D50u;
OAZ_HD uint32_t temperature_draw(uint64_t seed, uint64_t game, uint32_t ply, uint32_t S) {
    const u32x4 w = philox(seed, (uint32_t)game, (uint32_t)(game >> 32), kTemperatureTag, ply);
    return (uint32_t)(((uint64_t)w.x * (uint64_t)S) >> 32);
}
// The child the rule draws at ply `ply` of game `game`, or -1 when it draws nothing (no child, or no visit: the
// pass or the arg-max of visits is then played as without temperature). One body for the host entry
// (oaz_temperature_pick); the kernels' wave form (wave_temperature_pick, oaz_kernels.hip) is this with a lane per
// child.
OAZ_HD int temperature_draw_child(uint64_t seed, uint64_t game, uint32_t ply, const uint32_t* visits, int K) {
    if (K <= 0) return -1;
    uint32_t S = 0;
    for (int j = 0; j < K; ++j) S += visits[j];
    if (S == 0) return -1;
    const uint32_t r = temperature_draw(seed, game, ply, S);
    uint32_t acc = 0;
    for (int j = 0; j < K; ++j) {
        acc += visits[j];
        if (acc > r) return j;
    }
    return -1;  // (never reached: r < S)
}

// ---- playout cap randomization (oaz_selfplay_set_playout_cap) ---------------------
// Ply `ply` of global game `game` is a full ply (searched with cfg.sims playouts and recorded) iff the high 16
// bits of word 0 of Philox(seed; game lo, game hi, 0x50434150 "PCAP", ply) are below P, the full share in
// 1/65 536; every other ply is a fast one (fast_sims playouts, played only). The temperature draw's generator
// and counter layout under a tag of its own (>= 2^24 as well: no root-noise word equals it).
constexpr uint32_t kPlayoutCapTag = 0x50434150u;
OAZ_HD bool playout_cap_full(uint64_t seed, uint64_t game, uint32_t ply, uint32_t P) {
    const u32x4 w = philox(seed, (uint32_t)game, (uint32_t)(game >> 32), kPlayoutCapTag, ply);
    return (w.x >> 16) < P;
}

// ---- left-right reflection -------------------------------------------------------
// The reflection in the c-file: square i -> R(i) = 5 (i / 5) + 4 - i % 5, and card k -> C[k], the card whose
// attack map is the reflected one: reflect_bits(ATTACK[c][k][f]) == ATTACK[c][C[k]][R(f)] for both colours and
// all 25 squares. The rules commute with it (start position, temples and attack maps are symmetric; the law is
// checked against the oracle in tests/test_reflect.py), so a self-play record (s, pi, z) has the equally valid
// record (R s, R pi, z). One body for the host entries (oaz_reflect_*_host), k_reflect_samples and the trainer's
// gather (k_gather): a permutation of bits and bytes with no arithmetic in it.
OAZ_HD constexpr int reflect_sq(int i) { return i < 25 ? i + 4 - 2 * (i % 5) : i; }  // 25 (the pass move) is fixed
// columns a..e of every row; bits 6..0 are no squares and stay where they are
OAZ_HD constexpr uint32_t reflect_bits(uint32_t b) {
    constexpr uint32_t a = 0x84210800u;  // the a-file: squares 0, 5, 10, 15, 20
    return ((b & a) >> 4) | ((b & (a >> 4)) << 4) | ((b & (a >> 1)) >> 2) | ((b & (a >> 3)) << 2) |
           (b & ((a >> 2) | 0x7Fu));
}
// C, derived from the attack table: nibble k of the result is the unique k' with the law above. 0 when some card
// has no partner or more than one (the static_assert below then fails).
constexpr uint64_t make_reflect_cards() {
    uint64_t packed = 0;
    for (int k = 0; k < 16; ++k) {
        int found = -1, n = 0;
        for (int k2 = 0; k2 < 16; ++k2) {
            bool same = true;
            for (int color = 0; color < 2 && same; ++color)
                for (int f = 0; f < 25 && same; ++f)
                    same = reflect_bits(kAttackHost.m[color][k][f]) == kAttackHost.m[color][k2][reflect_sq(f)];
            if (same) {
                found = k2;
                ++n;
            }
        }
        if (n != 1) return 0;
        packed |= (uint64_t)found << (4 * k);
    }
    return packed;
}
constexpr uint64_t kReflectCards = make_reflect_cards();  // 16 nibbles: a scalar, so device code reads no table
OAZ_HD constexpr int reflect_card(int k) { return (int)((kReflectCards >> (4 * (k & 15))) & 15u); }
constexpr bool reflect_cards_involution() {
    for (int k = 0; k < 16; ++k)
        if (reflect_card(reflect_card(k)) != k) return false;
    return true;
}
static_assert(reflect_cards_involution(), "the card reflection must be an involution");
// 0 Tiger 1 Dragon 3 Rabbit 2 Frog 4 Crab 5 Elephant 7 Rooster 6 Goose 8 Monkey 9 Mantis 10 Crane 12 Ox 11 Horse
// 13 Boar 15 Cobra 14 Eel
static_assert(kReflectCards == 0xEFDBCA9867542310ull, "Frog<->Rabbit, Goose<->Rooster, Horse<->Ox, Eel<->Cobra");

// the four card bytes of one little-endian word (oaz_state.cards[0..3]); nbytes = 1 for the word that holds
// cards[4], to_move and pad, whose upper bytes stay
OAZ_HD uint32_t reflect_card_word(uint32_t w, int nbytes) {
    uint32_t out = w;
    for (int i = 0; i < nbytes; ++i) {
        const uint32_t c = (w >> (8 * i)) & 0xFFu;
        out = (out & ~(0xFFu << (8 * i))) | ((uint32_t)reflect_card((int)c) << (8 * i));
    }
    return out;
}
OAZ_HD void reflect_state(const oaz_state& in, oaz_state& out) {
    oaz_state s = in;
    for (int c = 0; c < 2; ++c) {
        s.kings[c] = reflect_bits(in.kings[c]);
        s.pawns[c] = reflect_bits(in.pawns[c]);
    }
    for (int k = 0; k < 5; ++k) s.cards[k] = (uint8_t)reflect_card(in.cards[k]);
    out = s;
}
OAZ_HD bool reflect_state_ok(const oaz_state& s) {  // what reflect_card is defined on
    return s.cards[0] < 16 && s.cards[1] < 16 && s.cards[2] < 16 && s.cards[3] < 16 && s.cards[4] < 16;
}
// A record as 57 little-endian words: 0-3 the bitboards, 4 cards[0..3], 5 cards[4] | to_move | pad, 6-55 pi
// [2][25], 56 z. Word d of the reflected record is a function of one word of the record: which one,
constexpr int kSampleWords = 57;
static_assert(sizeof(oaz_sample) == 4 * kSampleWords && sizeof(oaz_state) == 24, "oaz_sample is 57 words");
OAZ_HD int reflect_sample_src(int d) {  // pi'[k][t] = pi[k][R(t)] (R is an involution); every other word stays
    return (d >= 6 && d < 56) ? 6 + ((d - 6) / 25) * 25 + reflect_sq((d - 6) % 25) : d;
}
// ... and what becomes of it
OAZ_HD uint32_t reflect_sample_word(int d, uint32_t w) {
    return d < 4 ? reflect_bits(w) : d == 4 ? reflect_card_word(w, 4) : d == 5 ? reflect_card_word(w, 1) : w;
}

OAZ_HD uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// HASH test evaluator: a deterministic stand-in for the NN whose outputs are exact in fp32
// on every device, so MCTS trees can be compared bit for bit ("Hard parts").
OAZ_HD uint64_t hash_state(const oaz_state& s) {
    uint64_t h = splitmix64((uint64_t)s.kings[0] | ((uint64_t)s.kings[1] << 32));
    h = splitmix64(h ^ ((uint64_t)s.pawns[0] | ((uint64_t)s.pawns[1] << 32)));
    const uint64_t c = (uint64_t)(s.cards[0] & 15) | ((uint64_t)(s.cards[1] & 15) << 4) |
                       ((uint64_t)(s.cards[2] & 15) << 8) | ((uint64_t)(s.cards[3] & 15) << 12) |
                       ((uint64_t)(s.cards[4] & 15) << 16) | ((uint64_t)(s.to_move & 1) << 20);
    return splitmix64(h ^ c);
}
OAZ_HD float hash_policy(uint64_t h, int i) {
    return (float)((splitmix64(h + (uint64_t)i) >> 40) + 1) * (1.0f / 16777216.0f);
}
OAZ_HD float hash_value(uint64_t h) {
    const int32_t v = (int32_t)(splitmix64(h ^ 0x5DEECE66Dull) >> 40) - 8388608;
    return (float)v * (1.0f / 8388608.0f);
}

// ---- alpha-beta static evaluation: onitama-game/src/ai/alpha_beta/evaluation.rs:24-110 ------------
// One body for the host entry (oaz_alphabeta_evaluate) and the search kernel (oaz_alphabeta.hip), integer
// only. The reference's quirks are kept, in closed form:
//   - king positions are get_msb (common/mod.rs:57-66), 1-based (square n -> n + 1, empty board -> 0), the
//     temples 0-based squares, and both go through convert_to_2d(v) = (v / 5, v % 5);
//   - distance() is the f32 Euclidean distance truncated to i32: every squared distance here is an integer
//     <= 41 (rows 0..5, columns 0..4), where (int)sqrtf is the exact integer floor root, counted below by
//     the squares 1, 4, 9, 16, 25, 36 it reaches;
//   - every own pawn adds distance(1, enemy king position) (the pawn's bit value 1, not its square), every
//     enemy pawn on a square without an own pawn (`else if`) distance(1, my king position); the two
//     king-to-king terms are equal and cancel;
//   - PIECE_SQUARE_TABLE[n] = 4 * ((2 - |row - 2|) + (2 - |col - 2|)), summed through row and column masks.
OAZ_HD int ab_msb_pos(uint32_t v) { return v ? 32 - __builtin_ctz(v) : 0; }
OAZ_HD int ab_distance(int from, int to) {
    const int dx = to / 5 - from / 5, dy = to % 5 - from % 5, d2 = dx * dx + dy * dy;
    return (d2 >= 1) + (d2 >= 4) + (d2 >= 9) + (d2 >= 16) + (d2 >= 25) + (d2 >= 36);
}
OAZ_HD int ab_pst_sum(uint32_t p) {
    constexpr uint32_t kRow = 0xF8000000u, kCol = 0x84210800u;  // row 0, column 0
    constexpr uint32_t r13 = (kRow >> 5) | (kRow >> 15), r2 = kRow >> 10, c13 = (kCol >> 1) | (kCol >> 3), c2 = kCol >> 2;
    return 4 * (__builtin_popcount(p & r13) + 2 * __builtin_popcount(p & r2) + __builtin_popcount(p & c13) +
                2 * __builtin_popcount(p & c2));
}
// Evaluation::evaluate(state, color, move_result); won = move_result is Some(RedWin | BlueWin)
OAZ_HD int32_t alphabeta_evaluate(const oaz_state& s, int color, bool won) {
    const bool blue = color != OAZ_RED;
    const int32_t sign = blue ? -1 : 1;
    if (won) return -sign * 10000;
    const uint32_t mk = blue ? s.kings[1] : s.kings[0], ek = blue ? s.kings[0] : s.kings[1];
    const uint32_t mp = blue ? s.pawns[1] : s.pawns[0], ep = blue ? s.pawns[0] : s.pawns[1];
    const int my_temple = blue ? kBlueTemple : kRedTemple, enemy_temple = blue ? kRedTemple : kBlueTemple;
    const int mkp = ab_msb_pos(mk), ekp = ab_msb_pos(ek);
    const int n_mp = __builtin_popcount(mp), n_ep = __builtin_popcount(ep);
    const uint32_t ep_seen = ep & ~mp;  // the 25-square loop looks at an enemy pawn only where no own pawn is
    const int32_t pieces = (n_mp - n_ep) * 10 + (__builtin_popcount(mk) - __builtin_popcount(ek)) * 10000;
    const int32_t temple = ab_distance(mkp, enemy_temple) - ab_distance(ekp, my_temple);
    const int32_t close = n_mp * ab_distance(1, ekp) - __builtin_popcount(ep_seen) * ab_distance(1, mkp);
    const int32_t squares = ab_pst_sum(mp) - ab_pst_sum(ep_seen);
    return sign * (pieces + temple + close + squares);
}

// ---- Random agent: onitama-game/src/ai/random.rs:11-43 ------------------------------------------------
// One body for the host entry (oaz_random_agent_move) and the arena kernel (oaz_arena.hip). The reference
// draws from thread_rng; here the two draws of game `game` at ply `ply` are words 0 and 1 of
// Philox(seed; game lo, game hi, 0x52414E44 "RAND", ply): card_idx = (w0 * 2) >> 32 of the mover's two cards,
// then move number (w1 * n) >> 32 of that card's n legal moves in generate_legal_moves order (from, to
// ascending: the order k_movegen emits for the slot). The quirks are kept (Q15): used_card_idx is 0 / 1 for
// Blue too, and without a legal move of the drawn card the move is a5 -> a4 with a pawn.
OAZ_HD void random_agent_move(const AttackTable& att, uint64_t seed, uint64_t game, uint32_t ply, const oaz_state& s,
                              oaz_move& out) {
    const u32x4 r = philox(seed, (uint32_t)game, (uint32_t)(game >> 32), 0x52414E44u, ply);
    const int card_idx = (int)(((uint64_t)r.x * 2u) >> 32);
    const bool blue = (s.to_move & 1) != 0;
    const uint32_t pawns = blue ? s.pawns[1] : s.pawns[0], king = blue ? s.kings[1] : s.kings[0];
    const uint32_t own = (pawns | king) & 0xFFFFFF80u;  // squares 0..24 only: they index the table
    const uint32_t* row = att.m[blue ? 1 : 0][state_card(s, (blue ? 2 : 0) + card_idx) & 15];
    uint32_t n = 0;
    for (uint32_t o = own; o;) {
        const int from = __builtin_clz(o);
        o &= ~sq_bit(from);
        n += (uint32_t)__builtin_popcount(row[from] & ~own);
    }
    out.from = 0;
    out.to = 5;
    out.piece = OAZ_PAWN;
    out.slot = (uint8_t)card_idx;
    if (n == 0) return;
    uint32_t k = (uint32_t)(((uint64_t)r.y * (uint64_t)n) >> 32);
    for (uint32_t o = own; o;) {
        const int from = __builtin_clz(o);
        o &= ~sq_bit(from);
        uint32_t m = row[from] & ~own;
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        if (k >= c) {
            k -= c;
            continue;
        }
        for (; k; --k) m &= ~sq_bit(__builtin_clz(m));
        out.from = (uint8_t)from;
        out.to = (uint8_t)__builtin_clz(m);
        out.piece = (uint8_t)((pawns & sq_bit(from)) ? OAZ_PAWN : OAZ_KING);
        return;
    }
}

// f64::total_cmp key (argmax ties and signed zeros as Rust orders them)
OAZ_HD int64_t total_key(double x) {
    int64_t i = (int64_t)__builtin_bit_cast(uint64_t, x);
    i ^= (int64_t)(((uint64_t)(i >> 63)) >> 1);
    return i;
}

}  // namespace oaz
