// hs_join.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the plain path's iteration (neuron_poker_amd/csrc/mcq_device.hpp: mcq_iteration_sum) with the
// instantiation NAMED by the caller: the number of opponents and of table cards to come as template arguments (or -1:
// counted at run time), both accumulators, both dealing laws.  tests/hostsim_diet and tests/hostsim_ways reach the straight
// forms only through the dispatch of mcq_iterations_sum; here every form in which an opponent pair joins its hand one pair
// late -- 1 to 7 opponents x 5, 2, 1 cards to come or a run-time count, 8 and 9 opponents with a run-time count -- and the
// general form, which keeps the old order, are walked lane by lane as the bulk kernel walks them (one stream of
// MCQ_STREAM_ITERS iterations per lane) and folded into the words of an mcq_result / mcq_result_ways row.
#include "../hostsim/hs_walk.hpp"

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc>.  nopp, ndeal: the template arguments, -1 = counted at run
// time; a value >= 0 must be the query's own (MCQ_EINVAL otherwise, and for a pair the product does not instantiate).
// uniform != 0: the uniform dealing law.  ways != 0: the split-pot accumulator, row = 22 words; else 13 words.
extern "C" int hs_join_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways,
                           uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    return hs::for_form<hs::AllForms>(uniform, ways, nopp, ndeal, [&](auto form) {
        typedef decltype(form) F;
        const hs::BaseDeck bd(*q);
        const McqDeckAoS deck = bd.aos();
        const McqSumTabs tabs = mcq_sum_tabs_of(hs::luts().tf);
        return F::walk(bd.qc, q->runs, seed, qid, row, [&](typename F::Draws &dr, typename F::Acc &acc) {
            mcq_iteration_sum<typename F::Draws, F::kNopp, F::kNdeal, typename F::Acc>(bd.qc, dr, deck, tabs, acc);
        });
    });
}
