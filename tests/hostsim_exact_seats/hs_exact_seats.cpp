// hs_exact_seats.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the per-seat lane code of the extended exact enumeration (neuron_poker_amd/csrc/mcq_exact_ext.hpp:
// mcq_exact_ext_level_seats, mcq_exact_ext_pass_seats, mcq_exact_ext_seats_word) for the HOST compiler and walks
// mcq_exact_ext_kernel<1, MCQ_ROW_SEATS>'s decomposition sequentially: completion by completion, the 64 lanes one after the
// other, their three sums added as the wave adds them, then word l of the row by lane l.  A record without a random
// opponent is walked as mcq_exact_ext_kernel<0, MCQ_ROW_SEATS> walks it (mcq_exact_ext_lone_seats).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_ext.hpp"

// -> 0, or the refusal: MCQ_XX_* (1..4), 5 = the range cannot be dealt, 6 = two random opponents.  weights: 32 words.
extern "C" int hs_exact_ext_seats(const mcq_query *q, const mcq_query_ext *x, int law, uint64_t *weights) {
    const McqTables &t = hs::luts();
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    const int why = mcq_exact_ext_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e, r_id);
    if (!mcq_exact_ext_dealable(e, r_id)) return 5;
    if (e.b.n_opp > 1u) return 6;
    uint64_t row[32];
    memset(row, 0, sizeof row);
    const uint32_t n_boards = mcq_exact_binom(e.b.L, e.b.k);
    if (e.b.n_opp == 0u) {
        for (uint32_t board = 0; board < n_boards; board++) {
            uint32_t level, k;
            if (!mcq_exact_ext_lone_seats(e, board, t.sel8, t.tf, t.tops, t.sd, level, k)) continue;
            const uint32_t inc = mcq_seat_increment(k);
            row[0] += 1u;
            for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
                if (!((level >> s) & 1u)) continue;
                row[2u + 3u * s] += (inc >> MCQ_SEAT_WIN_SHIFT) & 1u;
                row[3u + 3u * s] += (inc >> MCQ_SEAT_TIE_SHIFT) & 1u;
                row[4u + 3u * s] += inc & 0xFFFFu;
            }
        }
        memcpy(weights, row, sizeof row);
        return 0;
    }
    std::vector<uint8_t> cb_tab(MCQ_XX_MAX_RP);
    mcq_exact_ext_cb_table(e, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> pair_xy(MCQ_EXACT_PAIRS);
    for (uint32_t i = 0; i < MCQ_EXACT_PAIRS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    for (uint32_t board = 0; board < n_boards; board++) {
        uint32_t pos[5];
        mcq_exact_unrank(board, e.b.L, e.b.k, pos);
        McqExactBoard bd;
        mcq_exact_board(e.b, pos, t.sel8, t.tf, t.tops, t.sd, bd);
        uint32_t level;
        const uint32_t best = mcq_exact_ext_level_seats(e, bd, t.tf, t.tops, t.sd, level);
        McqCard rem_card[64];
        uint32_t rem_pos[64];
        for (uint32_t l = 0; l < e.m; l++) {
            rem_pos[l] = mcq_exact_rem_pos(pos, l);
            rem_card[l] = mcq_card(r_id[rem_pos[l]]);
        }
        uint32_t gt = 0, eq = 0, tot = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            McqExactAccSeats acc = {0, 0, 0};
            mcq_exact_ext_pass_seats(e, bd, best, lane, 64u, pair_xy.data(), rem_card, rem_pos, cb_tab.data(), t.tf, t.tops, t.sd,
                                     acc);
            gt += acc.gt;
            eq += acc.eq;
            tot += acc.tot;
        }
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t v = mcq_exact_ext_seats_word(lane, level, e.n_known, gt, eq, tot);
            if (lane < 32u) row[lane] += v;
            else if (v) return -1; /* the lanes beyond the row add nothing */
        }
    }
    memcpy(weights, row, sizeof row);
    return 0;
}
