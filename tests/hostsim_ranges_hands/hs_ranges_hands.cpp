// hs_ranges_hands.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// The per-hand entry of the weighted-range-per-seat Monte-Carlo path for the HOST compiler: the lane code
// (mcq_iteration_ranges, neuron_poker_amd/csrc/mcq_ranges.hpp) with the per-hand accumulator and the block tally of
// neuron_poker_amd/csrc/mcq_hands.hpp, walked in mcq_eval_ranges_hands_kernel's order -- block by block over the cost
// axis, a block's records one after the other, the tasks of a record's piece to the waves in rounds, the table of hands
// (uint32 words, as in LDS) flushed to the rows by the kernel's rule.  What the kernel's threads do at once happens here
// one behind the other; the sums are integers, so the order does not show.
#include <string.h>

#include "../../neuron_poker_amd/csrc/mcq_ranges.hpp"
#include "../hostsim/hs_walk.hpp"
#include "hs_hands.hpp"

extern "C" {

// A batch of n records (seat_table [n][10], tables [n_tables][1326], trials [n]: the records' prices, 1 .. 256, as the
// host library estimates them: scheduling only) on `grid` blocks of `waves` waves, watched seat `seat`.
// out: [n] rows of 32 words, hands: [n][1326] rows of 4 words.  -> 0; MCQ_EINVAL (-1) for what the library refuses before a
// launch; 2 = the failure marker (an iteration without an accepted trial).  flushes (may be null): flushes in the middle
// of a record's piece, summed over the blocks.
int hs_ranges_hands_run(const mcq_query *q, uint32_t n, const uint32_t *seat_table, const uint16_t *tables, uint32_t n_tables,
                        const uint32_t *trials, uint64_t seed, uint64_t first_qid, uint32_t seat, uint32_t grid, uint32_t waves,
                        mcq_result_seats *out, mcq_hand_row *hands, uint32_t *flushes) {
    typedef McqLaneAccSeatsHands<hs::TableAdd> Acc;
    if (grid == 0u || waves == 0u || waves > MCQ_HT_BLOCK_WAVES || seat >= MCQ_MAX_SEATS) return MCQ_EINVAL;
    std::vector<uint32_t> cum((size_t)n_tables * MCQ_RG_CUM_STRIDE);
    for (uint32_t t = 0; t < n_tables; t++) mcq_ranges_prefix(tables + (size_t)t * MCQ_HAND_ROWS, cum.data() + (size_t)t * MCQ_RG_CUM_STRIDE);
    std::vector<uint64_t> prefix(n + 1u, 0ull);
    for (uint32_t i = 0; i < n; i++) { /* what the library refuses, and the cost prefix as mcq_prep_ranges_kernel lays it */
        const McqQueryWords qw = mcq_query_words(q[i]);
        if (!mcq_ranges_query_valid(qw) || seat >= qw.n_players() || trials[i] == 0u || trials[i] > MCQ_RG_MAX_PRICE) return MCQ_EINVAL;
        const uint64_t bm = mcq_ranges_board_mask(qw);
        for (uint32_t s = 0; s < qw.n_players(); s++) {
            if (seat_table[(size_t)i * 10u + s] >= n_tables) return MCQ_EINVAL;
            const uint16_t *w = tables + (size_t)seat_table[(size_t)i * 10u + s] * MCQ_HAND_ROWS;
            bool any = false;
            for (uint32_t b = 1; b < 52u; b++)
                for (uint32_t a = 0; a < b; a++)
                    any = any || (w[MCQ_HAND_INDEX(a, b)] != 0 && !((bm >> a) & 1u) && !((bm >> b) & 1u));
            if (!any) return MCQ_EINVAL;
        }
        prefix[i + 1u] = prefix[i] + (uint64_t)mcq_ranges_task_count(qw) * (mcq_ranges_task_weight(qw) * trials[i]);
    }
    const McqTables &t = hs::luts();
    McqCard cards[64];
    for (uint32_t c = 0; c < 64; c++) cards[c] = mcq_card(c < 52 ? c : 0);
    memset(out, 0, (size_t)n * sizeof(*out));
    memset(hands, 0, (size_t)n * MCQ_HAND_ROWS * sizeof(*hands));
    for (uint32_t i = 0; i < n; i++) out[i].runs = q[i].runs;
    uint32_t n_flushes = 0;
    bool failed = false;
    const uint64_t total = prefix[n];
    std::vector<uint32_t> table(MCQ_HT_TABLE_WORDS, 0u); /* clear at the start of a block and behind every flush */
    for (uint32_t blk = 0; blk < grid; blk++) {
        const uint64_t blo = total * blk / grid, bhi = total * (blk + 1ull) / grid;
        for (uint32_t qi = 0; qi < n; qi++) { /* (a record outside the block's piece has no task in it) */
            const McqQueryWords qw = mcq_query_words(q[qi]);
            const uint32_t weight = mcq_ranges_task_weight(qw) * trials[qi];
            const McqHandsPiece piece = mcq_hands_piece(prefix[qi], weight, mcq_ranges_task_count(qw), blo, bhi);
            const uint32_t rounds = mcq_hands_rounds(piece, waves);
            if (rounds == 0u) continue;
            McqRangesCtx qc;
            mcq_ranges_ctx(qw, qc);
            McqRangesWaveCtx wc;
            memset(&wc, 0, sizeof wc);
            for (uint32_t s = 0; s < qc.n_players; s++) {
                wc.cum[s] = cum.data() + (size_t)seat_table[(size_t)qi * 10u + s] * MCQ_RG_CUM_STRIDE;
                wc.total[s] = mcq_ranges_seat_total(wc.cum[s]);
            }
            uint64_t *rows = reinterpret_cast<uint64_t *>(hands + (size_t)qi * MCQ_HAND_ROWS);
            uint16_t ids[MCQ_MAX_SEATS];
            uint32_t since = 0;
            for (uint32_t round = 0; round < rounds; round++) {
                for (uint32_t wv = 0; wv < waves; wv++) {
                    const uint32_t task = piece.first + round * waves + wv;
                    if (task >= piece.end) continue;
                    for (uint32_t lane = 0; lane < 64u; lane++) {
                        Acc acc = {};
                        acc.add.table = table.data();
                        acc.watched = seat;
                        const uint32_t stream = task * MCQ_WAVE + lane;
                        const uint64_t it0 = (uint64_t)stream * MCQ_STREAM_ITERS;
                        if (it0 < qc.runs) {
                            McqExtCtrDraws dr;
                            dr.start(seed, first_qid + qi, stream);
                            const uint64_t left = (uint64_t)qc.runs - it0;
                            const uint32_t cnt = (uint32_t)(left < MCQ_STREAM_ITERS ? left : MCQ_STREAM_ITERS);
                            for (uint32_t j = 0; j < cnt && !failed; j++)
                                failed = !mcq_iteration_ranges<McqExtCtrDraws, false, Acc>(qc, wc, dr, cards, t.sel8, ids, 1, t.tf, t.tops, t.sd, acc);
                        }
                        if (failed) return 2;
                        mcq_tally_fold(acc, reinterpret_cast<uint64_t *>(out + qi));
                    }
                }
                since++;
                if (mcq_hands_flush_due(since, rounds - 1u - round)) {
                    hs::flush(table, 64u * waves, rows);
                    since = 0;
                    n_flushes++;
                }
            }
            hs::flush(table, 64u * waves, rows);
        }
    }
    if (flushes) *flushes = n_flushes;
    return MCQ_OK;
}

// the flush bound on its own (hs_hands.hpp): -> the flushes before the end
uint32_t hs_hands_drive(uint32_t a, uint32_t b, uint32_t inc, uint64_t n_adds, int with_flush, uint64_t *row, uint32_t *other_words) {
    return hs::drive(a, b, inc, n_adds, with_flush != 0, row, other_words);
}

// the constants of mcq_hands.hpp: the table's words, a round's iterations, the rounds between two flushes, the unit
void hs_hands_constants(uint32_t *out) {
    out[0] = MCQ_HT_TABLE_WORDS;
    out[1] = MCQ_HT_ROUND_ITERS;
    out[2] = MCQ_HT_FLUSH_ROUNDS;
    out[3] = MCQ_SHARE_UNIT;
}

// mcq_seat_increment's word for k hands level
uint32_t hs_hands_increment(uint32_t k) { return mcq_seat_increment(k); }

// a record's tasks in a block's piece -> first, end, rounds
void hs_hands_piece(uint64_t pfx, uint32_t weight, uint32_t n_tasks, uint64_t blo, uint64_t bhi, uint32_t waves, uint32_t *out) {
    const McqHandsPiece p = mcq_hands_piece(pfx, weight, n_tasks, blo, bhi);
    out[0] = p.first;
    out[1] = p.end;
    out[2] = mcq_hands_rounds(p, waves);
}
}
