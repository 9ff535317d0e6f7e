// hs_diet.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the plain path's iteration (neuron_poker_amd/csrc/mcq_device.hpp: mcq_iterations) walked lane by lane as
// the bulk kernel walks it -- one stream of MCQ_STREAM_ITERS iterations per lane -- and folded into the thirteen words of
// an mcq_result row, so that the lane code can be compared with the oracle's CTR mode where no GPU exists.
#include <stdint.h>
#include <string.h>

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace {
McqTables g_tab;
bool g_init = false;
const McqTables &luts() {
    if (!g_init) { mcq_fill_tables(&g_tab); g_init = true; }
    return g_tab;
}
template <bool STRAIGHT>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    McqCard base[192]; /* the iteration's deck pointer is biased by -128 entries */
    for (uint32_t l = 0; l < 64; l++) base[128 + l] = mcq_base_entry(qc, l, t.sel8);
    memset(row, 0, 13 * sizeof(uint64_t));
    row[0] = q->runs;
    const uint32_t n_streams = (q->runs + MCQ_STREAM_ITERS - 1) / MCQ_STREAM_ITERS;
    for (uint32_t s = 0; s < n_streams; s++) {
        McqCtrDraws dr;
        dr.start(seed, qid, s);
        McqLaneAcc acc = {0, 0, 0};
        const uint64_t left = (uint64_t)q->runs - (uint64_t)s * MCQ_STREAM_ITERS;
        const uint32_t cnt = left < MCQ_STREAM_ITERS ? (uint32_t)left : MCQ_STREAM_ITERS;
        mcq_iterations<STRAIGHT>(qc, dr, base, t.tf, t.tops, t.sd, acc, cnt);
        acc.passes = cnt * qc.n_opp; /* one attempt per opponent, never re-drawn */
        mcq_tally_fold(acc, row);
    }
    return MCQ_OK;
}
}  // namespace

// row: runs, passes, win, tie, by_type[9]; straight != 0: the straight-line forms the bulk kernel runs, else the general form
extern "C" int hs_diet_run(const mcq_query *q, uint64_t seed, uint64_t qid, int straight, uint64_t *row) {
    return straight ? run<true>(q, seed, qid, row) : run<false>(q, seed, qid, row);
}
// what a card adds to a hand's rank sum, and the flush selector of a table of five cards (card ids)
extern "C" uint32_t hs_diet_card_sum(uint32_t c) { return mcq_card_sum(c).rb; }
extern "C" uint32_t hs_diet_psel(const uint8_t *cards, uint32_t n) {
    McqSumBoard b;
    b.clear();
    for (uint32_t i = 0; i < n; i++) b.add(mcq_card_sum(cards[i]));
    McqFlushSel fs;
    fs.from_board(b);
    return fs.psel;
}
