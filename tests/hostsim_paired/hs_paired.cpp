// hs_paired.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the paired count of the dealing in epochs (neuron_poker_amd/csrc/mcq_device.hpp: mcq_hole_count2, the
// biased registers of mcq_draw_epoch) with the switch NAMED by the caller: every entry takes `paired` and runs the
// instantiation with MCQ_COUNT_PAIRED's place in the template list set to 1 or 0, so one library holds both texts.
//   * hs_paired_count2: the primitive on explicit registers, beside mcq_hole_count on the same two (the second unbiased).
//   * hs_paired_plan: what the plan says about pairs (cost by both models, which registers are biased and from where).
//   * hs_paired_positions: explicit draws through mcq_draw_epoch<N, RULE, 0..n-1, PAIRED> -> base positions.
//   * hs_paired_run: one query through mcq_iteration_sum<Draws, nopp, ndeal, Acc, .., PAIRED> as the bulk kernel walks it.
//   * hs_paired_replay: parity mode, mcq_iterations_replay4 (the switch's default: what the product ships).
#include "../hostsim/hs_walk.hpp"

namespace {
// HS_PAIRED_LEAN (hs_main.cpp, the stand-alone program under the sanitizers): the plans of 7, 12, 15, 19 and 23 draws, and
// of the iterations a few forms -- 6-max with five to come and with a run-time count, eight and ten players -- so that the
// instrumented build does not take minutes.  Anything else is refused.
#ifdef HS_PAIRED_LEAN
typedef std::integer_sequence<int, 5, 10, 13, 17, 21> PlanSizes; /* 7, 12, 15, 19, 23 draws */
struct Forms {
    static constexpr bool has(bool uniform, bool ways, int nopp, int ndeal) {
        return !uniform && !ways && ((nopp == 5 && (ndeal == 5 || ndeal == -1)) || ((nopp == 7 || nopp == 9) && ndeal == -1));
    }
};
#else
typedef hs::AllPlanSizes PlanSizes;
typedef hs::StraightForms Forms;
#endif

template <int PAIRED>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, uint64_t *row) {
    return hs::for_form<Forms>(uniform, ways, nopp, ndeal, [&](auto form) {
        typedef decltype(form) F;
        const hs::BaseDeck bd(*q);
        const McqDeckAoS deck = bd.aos();
        const McqSumTabs tabs = mcq_sum_tabs_of(hs::luts().tf);
        return F::walk(bd.qc, q->runs, seed, qid, row, [&](typename F::Draws &dr, typename F::Acc &acc) {
            mcq_iteration_sum<typename F::Draws, F::kNopp, F::kNdeal, typename F::Acc, McqDeckAoS, MCQ_DEAL_RULE, (MCQ_HOLE_BY_SUIT != 0), PAIRED>(
                bd.qc, dr, deck, tabs, acc);
        });
    });
}
}  // namespace

extern "C" {

// the switch the product ships with
int hs_paired_default(void) { return MCQ_COUNT_PAIRED; }

// n rows: out[i] = what mcq_hole_count2(pb, h0, h1b) adds to 0; single[i] = what two mcq_hole_count add, the second on the
// register with the bias taken off again
void hs_paired_count2(uint64_t n, const uint32_t *pb, const uint32_t *h0, const uint32_t *h1b, uint32_t *out, uint32_t *single) {
    for (uint64_t i = 0; i < n; i++) {
        uint32_t k = 0;
        mcq_hole_count2(pb[i], h0[i], h1b[i], k);
        out[i] = k;
        k = 0;
        mcq_hole_count(pb[i], h0[i], k);
        mcq_hole_count(pb[i], h1b[i] - MCQ_HOLE_BIAS, k);
        single[i] = k;
    }
}

// out[15]: n_epochs, cost by the model, cost with pairs, registers 0..5 (0 plain, 1 biased by its pair draw, 2 biased by its
// first scan), holes of epochs 0..5
int hs_paired_plan(int n_plan, int rule, int *out) {
    return hs::for_rule(rule, [&](auto r) {
        return hs::for_plan_size(n_plan, [&](auto n) {
            const McqDealPlan pl = mcq_deal_plan(decltype(n)::value, decltype(r)::value);
            out[0] = pl.n_epochs;
            out[1] = mcq_plan_cost(pl);
            out[2] = mcq_plan_cost_paired(pl);
            for (int g = 0; g < MCQ_PLAN_REGS; g++) out[3 + g] = 0;
            for (int e = 0; e < pl.n_epochs; e++) {
                const int holes = mcq_plan_holes(pl, e);
                for (int i = 0; pl.reg0[e] + i < pl.reg0[e + 1]; i++) /* 0 plain, 1 biased by its pair draw, 2 by its first scan */
                    out[3 + pl.reg0[e] + i] = !mcq_plan_biased(holes, i) ? 0 : mcq_plan_biased_by_pair(holes, i) ? 1 : 2;
                out[9 + e] = holes;
            }
            return (int)MCQ_OK;
        }, PlanSizes());
    });
}

// draws[rows][n] (r, unbiased) through the first n draws of the plan (n_plan, rule) -> pos[rows][n], base positions
int hs_paired_positions(int n_plan, int rule, int paired, int n, const uint8_t *draws, uint64_t rows, uint8_t *pos) {
    return paired ? hs::positions<PlanSizes, 1>(n_plan, rule, n, draws, rows, pos) : hs::positions<PlanSizes, 0>(n_plan, rule, n, draws, rows, pos);
}

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc, .., paired> under the product's rule, nopp >= 1; ndeal -1 =
// counted at run time.  uniform != 0: the uniform dealing law.  ways != 0: row = 22 words; else 13 words.
int hs_paired_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, int paired,
                  uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    return paired ? run<1>(q, seed, qid, nopp, ndeal, uniform, ways, row) : run<0>(q, seed, qid, nopp, ndeal, uniform, ways, row);
}

// Parity mode: the MT19937 stream of seed32 walked on the host, the draws four iterations per word through
// mcq_iterations_replay4 (1-5 opponents: its straight forms).  row = 13 words.
int hs_paired_replay(const mcq_query *q, uint32_t seed32, uint64_t *row) { return hs::replay_row<McqLaneAcc, false>(q, seed32, row); }
}
