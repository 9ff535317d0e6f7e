// hs_join.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the plain path's iteration (neuron_poker_amd/csrc/mcq_device.hpp: mcq_iteration_sum) with the
// instantiation NAMED by the caller: the number of opponents and of table cards to come as template arguments (or -1:
// counted at run time), both accumulators, both dealing laws.  tests/hostsim_diet and tests/hostsim_ways reach the straight
// forms only through the dispatch of mcq_iterations_sum; here every form in which an opponent pair joins its hand one pair
// late -- 1 to 7 opponents x 5, 2, 1 cards to come or a run-time count, 8 and 9 opponents with a run-time count -- and the
// general form, which keeps the old order, are walked lane by lane as the bulk kernel walks them (one stream of
// MCQ_STREAM_ITERS iterations per lane) and folded into the words of an mcq_result / mcq_result_ways row.
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

template <class Draws, class Acc, int NOPP, int NDEAL>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    if ((NOPP >= 0 && qc.n_opp != (uint32_t)NOPP) || (NDEAL >= 0 && qc.n_deal != (uint32_t)NDEAL)) return MCQ_EINVAL;
    McqCard base[192]; /* the iteration's deck pointer is biased by -128 entries */
    memset(base, 0, sizeof(base));
    for (uint32_t l = 0; l < 64; l++) base[128 + l] = mcq_base_entry(qc, l, t.sel8);
    const McqDeckAoS deck = {base};
    const McqSumTabs tabs = mcq_sum_tabs_of(t.tf);
    memset(row, 0, (Acc::kWays ? 22 : 13) * sizeof(uint64_t));
    row[0] = q->runs;
    const uint32_t n_streams = (q->runs + MCQ_STREAM_ITERS - 1) / MCQ_STREAM_ITERS;
    for (uint32_t s = 0; s < n_streams; s++) {
        Draws dr;
        dr.start(seed, qid, s);
        Acc acc = {};
        const uint64_t left = (uint64_t)q->runs - (uint64_t)s * MCQ_STREAM_ITERS;
        const uint32_t cnt = left < MCQ_STREAM_ITERS ? (uint32_t)left : MCQ_STREAM_ITERS;
        for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, NOPP, NDEAL, Acc>(qc, dr, deck, tabs, acc);
        row[1] += (uint64_t)cnt * qc.n_opp; /* passes: one attempt per opponent, never re-drawn */
        mcq_tally_fold(acc, row);
    }
    return MCQ_OK;
}

template <class Draws, class Acc, int NOPP>
int by_deal(int ndeal, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if (ndeal == -1) return run<Draws, Acc, NOPP, -1>(q, seed, qid, row);
    if constexpr (NOPP >= 1 && NOPP <= 7) { /* the instantiations mcq_iterations_sum has */
        if (ndeal == 5) return run<Draws, Acc, NOPP, 5>(q, seed, qid, row);
        if (ndeal == 2) return run<Draws, Acc, NOPP, 2>(q, seed, qid, row);
        if (ndeal == 1) return run<Draws, Acc, NOPP, 1>(q, seed, qid, row);
    }
    return MCQ_EINVAL;
}
template <class Draws, class Acc>
int by_opp(int nopp, int ndeal, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    switch (nopp) {
        case -1: return by_deal<Draws, Acc, -1>(ndeal, q, seed, qid, row);
        case 1: return by_deal<Draws, Acc, 1>(ndeal, q, seed, qid, row);
        case 2: return by_deal<Draws, Acc, 2>(ndeal, q, seed, qid, row);
        case 3: return by_deal<Draws, Acc, 3>(ndeal, q, seed, qid, row);
        case 4: return by_deal<Draws, Acc, 4>(ndeal, q, seed, qid, row);
        case 5: return by_deal<Draws, Acc, 5>(ndeal, q, seed, qid, row);
        case 6: return by_deal<Draws, Acc, 6>(ndeal, q, seed, qid, row);
        case 7: return by_deal<Draws, Acc, 7>(ndeal, q, seed, qid, row);
        case 8: return by_deal<Draws, Acc, 8>(ndeal, q, seed, qid, row);
        case 9: return by_deal<Draws, Acc, 9>(ndeal, q, seed, qid, row);
        default: return MCQ_EINVAL;
    }
}
}  // namespace

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc>.  nopp, ndeal: the template arguments, -1 = counted at run
// time; a value >= 0 must be the query's own (MCQ_EINVAL otherwise, and for a pair the product does not instantiate).
// uniform != 0: the uniform dealing law.  ways != 0: the split-pot accumulator, row = 22 words; else 13 words.
extern "C" int hs_join_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways,
                           uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    if (uniform)
        return ways ? by_opp<McqCtrDrawsUniform, McqLaneAccWays>(nopp, ndeal, q, seed, qid, row)
                    : by_opp<McqCtrDrawsUniform, McqLaneAcc>(nopp, ndeal, q, seed, qid, row);
    return ways ? by_opp<McqCtrDraws, McqLaneAccWays>(nopp, ndeal, q, seed, qid, row)
                : by_opp<McqCtrDraws, McqLaneAcc>(nopp, ndeal, q, seed, qid, row);
}
