// hs_ranges.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the product's lane code of the weighted-range-per-seat Monte-Carlo entry (mcq_iteration_ranges,
// neuron_poker_amd/csrc/mcq_ranges.hpp) for the HOST compiler and walks the kernel's task / lane decomposition
// sequentially, as tests/hostsim_seats does for the extended per-seat form: one McqLaneAccSeats per stream, unpacked into
// the 32-word row as WaveTallySeats unpacks it.  A deal hook (MCQ_RANGES_DEAL_HOOK, host builds only) hands back every
// iteration's hands and table cards.
#include <stdint.h>
#include <string.h>

#include <vector>

namespace {
thread_local uint8_t *g_hands = nullptr; /* the current iteration's record: n_players x 2 ids, then five table ids */
thread_local uint32_t g_players = 0, g_board = 0;
inline void hs_dealt(uint32_t h, uint32_t c1, uint32_t c2) {
    if (!g_hands) return;
    if (h >= 0x100u) g_hands[2u * g_players + g_board + (h - 0x100u)] = (uint8_t)c1; /* table card number h - 0x100 to come */
    else { g_hands[2u * h] = (uint8_t)c1; g_hands[2u * h + 1u] = (uint8_t)c2; }
}
}  // namespace
#define MCQ_RANGES_DEAL_HOOK(h, c1, c2) hs_dealt(h, c1, c2)

#include "../../neuron_poker_amd/csrc/mcq_ranges.hpp"
#include "../hostsim/hs_walk.hpp"

extern "C" {

// One record: the streams of (seed, qid), every iteration through mcq_iteration_ranges.  seat_table: ten table numbers,
// tables: n_tables x 1326 weights.  out: 32 words.  hands (may be null): runs x (2 n_players + 5) card ids.
// -> 0; MCQ_EINVAL (-1) for what the library refuses before a launch; 2 = the failure marker (no accepted trial).
int hs_ranges_run(const mcq_query *q, const uint32_t *seat_table, const uint16_t *tables, uint32_t n_tables, uint64_t seed,
                  uint64_t qid, mcq_result_seats *out, uint8_t *hands) {
    const McqQueryWords qw = mcq_query_words(*q);
    if (!mcq_ranges_query_valid(qw)) return MCQ_EINVAL;
    const uint64_t bm = mcq_ranges_board_mask(qw);
    std::vector<uint32_t> cum((size_t)n_tables * MCQ_RG_CUM_STRIDE);
    for (uint32_t t = 0; t < n_tables; t++) mcq_ranges_prefix(tables + (size_t)t * MCQ_HAND_ROWS, cum.data() + (size_t)t * MCQ_RG_CUM_STRIDE);
    McqRangesCtx qc;
    mcq_ranges_ctx(qw, qc);
    McqRangesWaveCtx wc;
    memset(&wc, 0, sizeof wc);
    for (uint32_t s = 0; s < qc.n_players; s++) {
        if (seat_table[s] >= n_tables) return MCQ_EINVAL;
        const uint16_t *w = tables + (size_t)seat_table[s] * MCQ_HAND_ROWS;
        bool any = false;
        for (uint32_t b = 1; b < 52u; b++)
            for (uint32_t a = 0; a < b; a++)
                any = any || (w[MCQ_HAND_INDEX(a, b)] != 0 && !((bm >> a) & 1u) && !((bm >> b) & 1u));
        if (!any) return MCQ_EINVAL;
        wc.cum[s] = cum.data() + (size_t)seat_table[s] * MCQ_RG_CUM_STRIDE;
        wc.total[s] = mcq_ranges_seat_total(wc.cum[s]);
    }
    const McqTables &t = hs::luts();
    McqCard cards[64];
    for (uint32_t c = 0; c < 64; c++) cards[c] = mcq_card(c < 52 ? c : 0);
    memset(out, 0, sizeof(*out));
    out->runs = q->runs;
    uint16_t ids[MCQ_MAX_SEATS];
    const uint32_t rec = 2u * q->n_players + 5u;
    g_players = q->n_players;
    g_board = q->n_board;
    struct Unhook { ~Unhook() { g_hands = nullptr; } } unhook;
    const uint64_t n_streams = ((uint64_t)q->runs + MCQ_STREAM_ITERS - 1u) / MCQ_STREAM_ITERS;
    for (uint64_t s = 0; s < n_streams; s++) { /* stream = task * 64 + lane */
        McqExtCtrDraws dr;
        dr.start(seed, qid, (uint32_t)s);
        McqLaneAccSeats acc = {};
        bool failed = false;
        for (uint32_t j = 0; j < MCQ_STREAM_ITERS && !failed; j++) {
            const uint64_t it = s * MCQ_STREAM_ITERS + j;
            if (it >= q->runs) break;
            if (hands) {
                g_hands = hands + it * rec;
                for (uint32_t k = 0; k < q->n_board; k++) g_hands[2u * q->n_players + k] = q->board[k];
            }
            failed = !mcq_iteration_ranges<McqExtCtrDraws, false, McqLaneAccSeats>(qc, wc, dr, cards, t.sel8, ids, 1, t.tf, t.tops, t.sd, acc);
        }
        if (failed) return 2;
        mcq_tally_fold(acc, reinterpret_cast<uint64_t *>(out));
    }
    return MCQ_OK;
}

/* the word -> hand mapping on its own: the hand (a | b << 8) that the draw word u selects from one table */
uint32_t hs_ranges_pick(const uint16_t *table, uint32_t u) {
    uint32_t cum[MCQ_RG_CUM_STRIDE];
    mcq_ranges_prefix(table, cum);
    const uint32_t t = mcq_mulhi(u, cum[MCQ_RG_TOTAL_WORD]);
    uint32_t i = 0;
    while (i < MCQ_HAND_ROWS - 1u && cum[i] <= t) i++; /* the specification, literally */
    uint32_t a, b;
    mcq_ranges_hand(i, a, b);
    return a | (b << 8);
}
}
