// hs_epochs.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the dealing in epochs (neuron_poker_amd/csrc/mcq_device.hpp: mcq_deal_plan, mcq_draw_epoch) and of the
// iteration that deals by it (mcq_iteration_sum with NOPP >= 1), with the instantiation NAMED by the caller.
//   * hs_epochs_plan: a plan as the lane code sees it (checkpoints, registers, cost by the model).
//   * hs_epochs_positions: explicit draws through mcq_draw_epoch<N, RULE, 0..n-1> in the order of an iteration -> base
//     positions, for every number of draws N a plan exists for and every rule; n < N is an iteration that stops early in
//     the plan (a form whose table cards to come are counted at run time deals by the plan of five).
//   * hs_epochs_run: one query through mcq_iteration_sum<Draws, nopp, ndeal, Acc> as the bulk kernel walks it, as
//     tests/hostsim_join does, under the rule the product ships (or rule 0: the dealing without plans).
//   * hs_epochs_replay: parity mode, the host's walk of the MT19937 stream and mcq_iterations_replay4.
#include "../hostsim/hs_walk.hpp"

namespace {
// HS_EPOCHS_LEAN (hs_main.cpp, the stand-alone program under the sanitizers): the plans of 3, 7, 12, 15 and 23 draws, and of
// the iterations a few forms, by the product's rule only -- one opponent and one card to come, 6-max with five to come and
// with a run-time count, ten players; split-pot rows under the reference law only -- so that the instrumented build does
// not take minutes.  Anything else is refused.
#ifdef HS_EPOCHS_LEAN
constexpr bool kLean = true;
typedef std::integer_sequence<int, 1, 5, 10, 13, 21> PlanSizes; /* 3, 7, 12, 15, 23 draws */
struct Forms {
    static constexpr bool has(bool uniform, bool ways, int nopp, int ndeal) {
        return !(uniform && ways) && ((nopp == 1 && ndeal == 1) || (nopp == 5 && (ndeal == 5 || ndeal == -1)) || (nopp == 9 && ndeal == -1));
    }
};
#else
constexpr bool kLean = false;
typedef hs::AllPlanSizes PlanSizes;
typedef hs::StraightForms Forms;
#endif

template <int RULE>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, uint64_t *row) {
    return hs::for_form<Forms>(uniform, ways, nopp, ndeal, [&](auto form) {
        typedef decltype(form) F;
        const hs::BaseDeck bd(*q);
        const McqDeckAoS deck = bd.aos();
        const McqSumTabs tabs = mcq_sum_tabs_of(hs::luts().tf);
        return F::walk(bd.qc, q->runs, seed, qid, row, [&](typename F::Draws &dr, typename F::Acc &acc) {
            mcq_iteration_sum<typename F::Draws, F::kNopp, F::kNdeal, typename F::Acc, McqDeckAoS, RULE>(bd.qc, dr, deck, tabs, acc);
        });
    });
}
}  // namespace

extern "C" {

// the rule the straight forms of the product deal by
int hs_epochs_rule(void) { return MCQ_DEAL_RULE; }

// out[17]: n_epochs, first[7], reg0[7], cost by the model, mcq_plan_valid
int hs_epochs_plan(int n_plan, int rule, int *out) {
    return hs::for_rule(rule, [&](auto r) {
        return hs::for_plan_size(n_plan, [&](auto n) {
            const McqDealPlan pl = mcq_deal_plan(decltype(n)::value, decltype(r)::value);
            out[0] = pl.n_epochs;
            for (int e = 0; e <= MCQ_PLAN_MAX_EPOCHS; e++) { out[1 + e] = pl.first[e]; out[8 + e] = pl.reg0[e]; }
            out[15] = mcq_plan_cost(pl);
            out[16] = mcq_plan_valid(pl) ? 1 : 0;
            return (int)MCQ_OK;
        }, PlanSizes());
    });
}

// draws[rows][n] (r, unbiased) through the first n draws of the plan (n_plan, rule) -> pos[rows][n], base positions
int hs_epochs_positions(int n_plan, int rule, int n, const uint8_t *draws, uint64_t rows, uint8_t *pos) {
    return hs::positions<PlanSizes>(n_plan, rule, n, draws, rows, pos);
}

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc>, nopp >= 1; ndeal -1 = counted at run time.  planned != 0:
// by the product's rule, else rule 0.  uniform != 0: the uniform dealing law.  ways != 0: row = 22 words; else 13 words.
int hs_epochs_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, int planned,
                  uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    if (planned) return run<MCQ_DEAL_RULE>(q, seed, qid, nopp, ndeal, uniform, ways, row);
    if constexpr (kLean) return MCQ_EINVAL;
    else return run<0>(q, seed, qid, nopp, ndeal, uniform, ways, row);
}

// Parity mode: the MT19937 stream of seed32 walked on the host, the draws four iterations per word through
// mcq_iterations_replay4 (1-5 opponents: its straight forms).  row = 13 words.
int hs_epochs_replay(const mcq_query *q, uint32_t seed32, uint64_t *row) { return hs::replay_row<McqLaneAcc, false>(q, seed32, row); }
}
