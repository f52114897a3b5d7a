/*
 * alphabeta_ref.c — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference's alpha-beta agent, written in plain C from the Rust text:
 *   onitama-game/src/ai/alpha_beta/mod.rs:35-183      (alpha_beta, generate_move)
 *   onitama-game/src/ai/alpha_beta/evaluation.rs:1-110 (Evaluation::evaluate, distance)
 *   onitama-game/src/common/mod.rs:1-66                (get_bit, count_bits, get_msb)
 * It keeps the reference's shape (recursion, a copy for `undo`, the two nested loops with the same
 * three `break 'br`) and takes its rules from the oracle library (orc_movegen, orc_make_move,
 * orc_deal_deck, orc_initial_state), which the reference's own KATs pin. It shares no code with the
 * product (csrc/): it is the checker of oaz_alphabeta_evaluate / oaz_alphabeta_search, and the
 * generator of tests/golden/alphabeta_kats.json (tools/make_alphabeta_kats.py).
 *
 * Defined where the reference is not (it panics in both):
 *   - a root without a legal move returns the pass move (from = to = 25, piece 0, slot = the mover's
 *     first card slot) with the untouched best_score (INT32_MIN for Red, INT32_MAX for Blue);
 *   - a root with legal moves of which none improves on that sentinel (every child returned it) returns
 *     its first legal move with the sentinel as score.
 */
#include <stdint.h>
#include <string.h>

#include "oaz_oracle.h"

#define ABREF_NONE 255 /* move_result: Option::None */

static const int32_t PIECE_SQUARE_TABLE[25] = {
    0, 4, 8,  4, 0, /**/ 4, 8, 12, 8, 4, /**/ 8, 12, 16, 12, 8, /**/ 4, 8, 12, 8, 4, /**/ 0, 4, 8, 4, 0,
};

static uint32_t get_bit(uint32_t x, int n) { return (x >> (31 - n)) & 1u; } /* common/mod.rs:2-4 */

static uint32_t count_bits(uint32_t value) { /* common/mod.rs:46-53 */
    uint32_t count = 0;
    while (value != 0) {
        count += 1;
        value &= value - 1;
    }
    return count;
}

static uint32_t get_msb(uint32_t value) { /* common/mod.rs:57-66: 1-based, 0 for an empty board */
    uint32_t pos = 0;
    while (value > 0) {
        pos += 1;
        value <<= 1;
    }
    return pos;
}

/* evaluation.rs:92-109 with Move::convert_to_2d (move.rs:28-32): (value / 5, value % 5); the f32
 * Euclidean distance truncated to i32. */
static int32_t distance(uint32_t from, uint32_t to) {
    const float fx = (float)(from / 5), fy = (float)(from % 5), tx = (float)(to / 5), ty = (float)(to % 5);
    return (int32_t)__builtin_sqrtf((tx - fx) * (tx - fx) + (ty - fy) * (ty - fy));
}

/* evaluation.rs:24-90; move_result = MoveResult or ABREF_NONE */
int32_t abref_evaluate(const oaz_state* state, int player_color, int move_result) {
    int32_t sign = 1;
    const int enemy_color = player_color ^ 1;
    if (player_color == OAZ_BLUE) sign = -1;
    if (move_result == OAZ_BLUE_WIN || move_result == OAZ_RED_WIN) return -sign * 10000;
    const uint32_t enemy_temple = player_color == OAZ_RED ? 2 : 22; /* BLUE_TEMPLE, RED_TEMPLE (state.rs:48-49) */
    const uint32_t my_temple = player_color == OAZ_RED ? 22 : 2;
    const uint32_t my_king = state->kings[player_color], enemy_king = state->kings[enemy_color];
    const uint32_t my_king_pos = get_msb(my_king), enemy_king_pos = get_msb(enemy_king);
    const uint32_t my_pawns = state->pawns[player_color], enemy_pawns = state->pawns[enemy_color];
    const int32_t my_piece_score_sum = (int32_t)(count_bits(my_pawns) * 10 + count_bits(my_king) * 10000);
    const int32_t enemy_piece_score_sum = (int32_t)(count_bits(enemy_pawns) * 10 + count_bits(enemy_king) * 10000);
    const int32_t enemy_distance_to_temple = distance(enemy_king_pos, my_temple);
    const int32_t my_distance_to_temple = distance(my_king_pos, enemy_temple);
    int32_t me_close_to_enemy_king = 0, enemies_close_to_my_king = 0, my_piece_square = 0, enemy_piece_square = 0;
    for (int n = 0; n < 25; n++) {
        const uint32_t my_pawn = get_bit(my_pawns, n), enemy_pawn = get_bit(enemy_pawns, n);
        if (my_pawn == 1) {
            me_close_to_enemy_king += distance(my_pawn, enemy_king_pos); /* the bit value, not the square */
            my_piece_square += PIECE_SQUARE_TABLE[n];
        } else if (enemy_pawn == 1) {
            enemies_close_to_my_king += distance(enemy_pawn, my_king_pos);
            enemy_piece_square += PIECE_SQUARE_TABLE[n];
        }
    }
    enemies_close_to_my_king += distance(enemy_king_pos, my_king_pos);
    me_close_to_enemy_king += distance(my_king_pos, enemy_king_pos);
    return sign * ((my_piece_score_sum - enemy_piece_score_sum) + (my_distance_to_temple - enemy_distance_to_temple) +
                   (me_close_to_enemy_king - enemies_close_to_my_king) + (my_piece_square - enemy_piece_square));
}

/* n evaluations: colour = s[i].to_move, move_result[i] (ABREF_NONE for None) */
void abref_evaluate_batch(const oaz_state* s, const uint8_t* move_result, int n, int32_t* out) {
    for (int i = 0; i < n; i++) out[i] = abref_evaluate(&s[i], s[i].to_move & 1, move_result[i]);
}

typedef struct {
    int has_move;
    oaz_move best_move;
    int32_t best_score;
} calc_result;

static _Thread_local int64_t g_interior_without_move; /* interior nodes (depth > 0) without a legal move, last search */

/* mod.rs:36-132; game_state = (state, state->to_move) */
static calc_result alpha_beta(int depth, int max_depth, int32_t alpha, int32_t beta, oaz_state* game_state,
                              int move_result, int64_t* positions) {
    *positions += 1;
    const int player_color = game_state->to_move & 1;
    calc_result r;
    memset(&r, 0, sizeof(r));
    if (depth == max_depth || move_result == OAZ_BLUE_WIN || move_result == OAZ_RED_WIN) {
        r.best_score = abref_evaluate(game_state, player_color, move_result);
        return r;
    }
    const int cards[2] = {player_color == OAZ_RED ? 0 : 2, player_color == OAZ_RED ? 1 : 3}; /* deck.rs get_player_cards_idx */
    int32_t best_score = player_color == OAZ_RED ? INT32_MIN : INT32_MAX;
    oaz_move all[OAZ_MAX_MOVES];
    const int n_all = orc_movegen(game_state, player_color, all); /* card slot, from, to ascending */
    if (n_all == 0 && depth > 0) g_interior_without_move += 1;
    for (int ci = 0; ci < 2; ci++) {
        const int card_idx = cards[ci];
        for (int k = 0; k < n_all; k++) { /* 'br: the moves of this card */
            if (all[k].slot != card_idx) continue;
            const oaz_move done_move = all[k];
            const oaz_state undo = *game_state;
            const int result = orc_make_move(game_state, &done_move, player_color); /* GameState::progress */
            game_state->to_move ^= 1;
            const calc_result calc = alpha_beta(depth + 1, max_depth, alpha, beta, game_state, result, positions);
            const int32_t score = calc.best_score;
            *game_state = undo;
            if (player_color == OAZ_RED) {
                if (score > best_score) {
                    best_score = score;
                    r.best_move = done_move;
                    r.has_move = 1;
                }
                if (score >= beta) break;
                alpha = alpha > score ? alpha : score;
            } else {
                if (score < best_score) {
                    best_score = score;
                    r.best_move = done_move;
                    r.has_move = 1;
                }
                if (score <= alpha) break;
                beta = beta < score ? beta : score;
            }
            if (alpha >= beta) break;
        }
    }
    r.best_score = best_score;
    if (depth == 0 && !r.has_move) { /* the reference panics here (mod.rs:165-167) */
        if (n_all > 0) {
            r.best_move = all[0];
        } else {
            r.best_move.from = 25;
            r.best_move.to = 25;
            r.best_move.piece = 0;
            r.best_move.slot = (uint8_t)cards[0];
        }
    }
    return r;
}

/* generate_move (mod.rs:136-170) not cut by the clock: iterations depth = 1 .. max_depth - 1 carry nothing
 * over and the last one is the result, so only that one is run; *positions counts its alpha_beta calls.
 * Returns 0, or -1 for max_depth < 2 (the reference's unwrap of None). */
int abref_search(const oaz_state* root, int max_depth, oaz_move* out_move, int32_t* out_score, int64_t* positions,
                 int64_t* interior_without_move) {
    if (max_depth < 2) return -1;
    oaz_state gs = *root;
    int64_t pos = 0;
    g_interior_without_move = 0;
    const calc_result result = alpha_beta(0, max_depth - 1, INT32_MIN, INT32_MAX, &gs, ABREF_NONE, &pos);
    *out_move = result.best_move;
    *out_score = result.best_score;
    if (positions) *positions = pos;
    if (interior_without_move) *interior_without_move = g_interior_without_move;
    return 0;
}

/* n searches, one after the other (the last iteration of each, and its positions) */
int abref_search_batch(const oaz_state* roots, int n, int max_depth, oaz_move* out_move, int32_t* out_score,
                       int64_t* positions) {
    for (int i = 0; i < n; i++) {
        const int rc = abref_search(&roots[i], max_depth, &out_move[i], &out_score[i], &positions[i], NULL);
        if (rc != 0) return rc;
    }
    return 0;
}

/* One AlphaBeta-vs-AlphaBeta game under fight's loop (alphazero-training/src/evaluator.rs:373-389) from
 * the deal of (deal_seed, game): *result = the last MoveResult, *plies = moves played (max_plies 150 gives
 * the 152-ply cut), moves[0 .. *plies) the moves (cap entries at least max_plies + 2). A pass (a root
 * without a legal move) swaps the named card with the neutral one and hands the turn over
 * (State::pass, state.rs:139-142). */
int abref_play(uint64_t deal_seed, uint64_t game, int max_depth, int max_plies, int* result, int* plies,
               oaz_move* moves, int cap) {
    uint8_t deck[5];
    orc_deal_deck(deal_seed, game, deck);
    oaz_state s;
    orc_initial_state(deck, &s);
    int progress = OAZ_IN_PROGRESS, n = 0;
    while (!(progress == OAZ_RED_WIN || progress == OAZ_BLUE_WIN)) {
        oaz_move mv;
        int32_t score;
        if (abref_search(&s, max_depth, &mv, &score, NULL, NULL) != 0) return -1;
        if (n >= cap) return -2;
        moves[n++] = mv;
        if (mv.from >= 25) {
            const uint8_t t = s.cards[mv.slot];
            s.cards[mv.slot] = s.cards[4];
            s.cards[4] = t;
            progress = OAZ_IN_PROGRESS;
        } else {
            progress = orc_make_move(&s, &mv, s.to_move & 1);
        }
        s.to_move ^= 1;
        if (max_plies < 0) break;
        max_plies -= 1;
    }
    *result = progress;
    *plies = n;
    return 0;
}
