// hs_diet.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the plain path's iteration (neuron_poker_amd/csrc/mcq_device.hpp: mcq_iterations) walked lane by lane as
// the bulk kernel walks it -- one stream of MCQ_STREAM_ITERS iterations per lane -- and folded into the thirteen words of
// an mcq_result row, so that the lane code can be compared with the oracle's CTR mode where no GPU exists.
#include "../hostsim/hs_walk.hpp"

namespace {
template <bool STRAIGHT>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = hs::luts();
    const hs::BaseDeck bd(*q);
    hs::walk_streams<McqCtrDraws, McqLaneAcc>(bd.qc, q->runs, seed, qid, row, [&](McqCtrDraws &dr, McqLaneAcc &acc, uint32_t cnt) {
        mcq_iterations<STRAIGHT>(bd.qc, dr, bd.card, t.tf, t.tops, t.sd, acc, cnt);
    });
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
