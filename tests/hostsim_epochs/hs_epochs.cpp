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
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_replay.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace {
// HS_EPOCHS_LEAN (hs_main.cpp, the stand-alone program under the sanitizers): the plans of 3, 7, 12, 15 and 23 draws, and of
// the iterations a few forms, by the product's rule only -- one opponent and one card to come, 6-max with five to come and
// with a run-time count, ten players; split-pot rows under the reference law only -- so that the instrumented build does
// not take minutes.  Anything else is refused.
#ifdef HS_EPOCHS_LEAN
constexpr bool kLean = true;
#else
constexpr bool kLean = false;
#endif
McqTables g_tab;
bool g_init = false;
const McqTables &luts() {
    if (!g_init) { mcq_fill_tables(&g_tab); g_init = true; }
    return g_tab;
}

// ---- positions
template <int N, int RULE, int D>
void draw_from(const uint8_t *r, int n, uint32_t (&E)[MCQ_PLAN_REGS], uint8_t *pos) {
    if constexpr (D < N) {
        if (D >= n) return;
        pos[D] = (uint8_t)(mcq_draw_epoch<N, RULE, D>(r[D] | 0x80u, E) - 128u);
        draw_from<N, RULE, D + 1>(r, n, E, pos);
    }
}
template <int N, int RULE>
int positions(int n, const uint8_t *draws, uint64_t rows, uint8_t *pos) {
    if (n < 1 || n > N) return MCQ_EINVAL;
    for (uint64_t i = 0; i < rows; i++) {
        uint32_t E[MCQ_PLAN_REGS] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL,
                                     MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
        draw_from<N, RULE, 0>(draws + i * (uint64_t)n, n, E, pos + i * (uint64_t)n);
    }
    return MCQ_OK;
}
template <int RULE, int... NS>
int positions_by_n(int n_plan, int n, const uint8_t *draws, uint64_t rows, uint8_t *pos, std::integer_sequence<int, NS...>) {
    int rc = MCQ_EINVAL;
    (void)((n_plan == NS + 2 ? (rc = positions<NS + 2, RULE>(n, draws, rows, pos), true) : false) || ...);
    return rc;
}
template <int RULE, int... NS>
int plan_by_n(int n_plan, int *out, std::integer_sequence<int, NS...>) {
    int rc = MCQ_EINVAL;
    auto put = [&](const McqDealPlan &pl) {
        out[0] = pl.n_epochs;
        for (int e = 0; e <= MCQ_PLAN_MAX_EPOCHS; e++) { out[1 + e] = pl.first[e]; out[8 + e] = pl.reg0[e]; }
        out[15] = mcq_plan_cost(pl);
        out[16] = mcq_plan_valid(pl) ? 1 : 0;
        rc = MCQ_OK;
        return true;
    };
    (void)((n_plan == NS + 2 ? put(mcq_deal_plan(NS + 2, RULE)) : false) || ...);
    return rc;
}
#ifdef HS_EPOCHS_LEAN
typedef std::integer_sequence<int, 1, 5, 10, 13, 21> PlanSizes; /* 3, 7, 12, 15, 23 draws */
#else
typedef std::make_integer_sequence<int, MCQ_PLAN_MAX_DRAWS - 1> PlanSizes; /* 2 .. 23 draws */
#endif

// ---- tallies
template <class Draws, class Acc, int NOPP, int NDEAL, int RULE>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    if (qc.n_opp != (uint32_t)NOPP || (NDEAL >= 0 && qc.n_deal != (uint32_t)NDEAL)) return MCQ_EINVAL;
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
        for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, NOPP, NDEAL, Acc, McqDeckAoS, RULE>(qc, dr, deck, tabs, acc);
        row[1] += (uint64_t)cnt * qc.n_opp; /* passes: one attempt per opponent, never re-drawn */
        mcq_tally_fold(acc, row);
    }
    return MCQ_OK;
}
template <class Draws, class Acc, int NOPP, int RULE>
int by_deal(int ndeal, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if constexpr (kLean) {
        if constexpr (NOPP == 1) { if (ndeal == 1) return run<Draws, Acc, 1, 1, RULE>(q, seed, qid, row); }
        if constexpr (NOPP == 5) { if (ndeal == 5) return run<Draws, Acc, 5, 5, RULE>(q, seed, qid, row); }
        if constexpr (NOPP == 5 || NOPP == 9) { if (ndeal == -1) return run<Draws, Acc, NOPP, -1, RULE>(q, seed, qid, row); }
        return MCQ_EINVAL;
    }
    if (ndeal == -1) return run<Draws, Acc, NOPP, -1, RULE>(q, seed, qid, row);
    if constexpr (NOPP <= 7) { /* the instantiations mcq_iterations_sum has */
        if (ndeal == 5) return run<Draws, Acc, NOPP, 5, RULE>(q, seed, qid, row);
        if (ndeal == 2) return run<Draws, Acc, NOPP, 2, RULE>(q, seed, qid, row);
        if (ndeal == 1) return run<Draws, Acc, NOPP, 1, RULE>(q, seed, qid, row);
    }
    return MCQ_EINVAL;
}
template <class Draws, class Acc, int RULE>
int by_opp(int nopp, int ndeal, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if constexpr (kLean) {
        if (nopp == 1) return by_deal<Draws, Acc, 1, RULE>(ndeal, q, seed, qid, row);
        if (nopp == 5) return by_deal<Draws, Acc, 5, RULE>(ndeal, q, seed, qid, row);
        if (nopp == 9) return by_deal<Draws, Acc, 9, RULE>(ndeal, q, seed, qid, row);
        return MCQ_EINVAL;
    } else switch (nopp) {
        case 1: return by_deal<Draws, Acc, 1, RULE>(ndeal, q, seed, qid, row);
        case 2: return by_deal<Draws, Acc, 2, RULE>(ndeal, q, seed, qid, row);
        case 3: return by_deal<Draws, Acc, 3, RULE>(ndeal, q, seed, qid, row);
        case 4: return by_deal<Draws, Acc, 4, RULE>(ndeal, q, seed, qid, row);
        case 5: return by_deal<Draws, Acc, 5, RULE>(ndeal, q, seed, qid, row);
        case 6: return by_deal<Draws, Acc, 6, RULE>(ndeal, q, seed, qid, row);
        case 7: return by_deal<Draws, Acc, 7, RULE>(ndeal, q, seed, qid, row);
        case 8: return by_deal<Draws, Acc, 8, RULE>(ndeal, q, seed, qid, row);
        case 9: return by_deal<Draws, Acc, 9, RULE>(ndeal, q, seed, qid, row);
        default: return MCQ_EINVAL;
    }
}
template <int RULE>
int by_law(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, uint64_t *row) {
    if constexpr (kLean) {
        if (uniform && ways) return MCQ_EINVAL;
        if (uniform) return by_opp<McqCtrDrawsUniform, McqLaneAcc, RULE>(nopp, ndeal, q, seed, qid, row);
    } else if (uniform)
        return ways ? by_opp<McqCtrDrawsUniform, McqLaneAccWays, RULE>(nopp, ndeal, q, seed, qid, row)
                    : by_opp<McqCtrDrawsUniform, McqLaneAcc, RULE>(nopp, ndeal, q, seed, qid, row);
    return ways ? by_opp<McqCtrDraws, McqLaneAccWays, RULE>(nopp, ndeal, q, seed, qid, row)
                : by_opp<McqCtrDraws, McqLaneAcc, RULE>(nopp, ndeal, q, seed, qid, row);
}
}  // namespace

extern "C" {

// the rule the straight forms of the product deal by
int hs_epochs_rule(void) { return MCQ_DEAL_RULE; }

// out[17]: n_epochs, first[7], reg0[7], cost by the model, mcq_plan_valid
int hs_epochs_plan(int n_plan, int rule, int *out) {
    switch (rule) {
        case 1: return plan_by_n<1>(n_plan, out, PlanSizes());
        case 2: return plan_by_n<2>(n_plan, out, PlanSizes());
        case 3: return plan_by_n<3>(n_plan, out, PlanSizes());
        case MCQ_DEAL_FULLREG: return plan_by_n<MCQ_DEAL_FULLREG>(n_plan, out, PlanSizes());
        default: return MCQ_EINVAL;
    }
}

// draws[rows][n] (r, unbiased) through the first n draws of the plan (n_plan, rule) -> pos[rows][n], base positions
int hs_epochs_positions(int n_plan, int rule, int n, const uint8_t *draws, uint64_t rows, uint8_t *pos) {
    switch (rule) {
        case 1: return positions_by_n<1>(n_plan, n, draws, rows, pos, PlanSizes());
        case 2: return positions_by_n<2>(n_plan, n, draws, rows, pos, PlanSizes());
        case 3: return positions_by_n<3>(n_plan, n, draws, rows, pos, PlanSizes());
        case MCQ_DEAL_FULLREG: return positions_by_n<MCQ_DEAL_FULLREG>(n_plan, n, draws, rows, pos, PlanSizes());
        default: return MCQ_EINVAL;
    }
}

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc>, nopp >= 1; ndeal -1 = counted at run time.  planned != 0:
// by the product's rule, else rule 0.  uniform != 0: the uniform dealing law.  ways != 0: row = 22 words; else 13 words.
int hs_epochs_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, int planned,
                  uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    if (planned) return by_law<MCQ_DEAL_RULE>(q, seed, qid, nopp, ndeal, uniform, ways, row);
    if constexpr (kLean) return MCQ_EINVAL;
    else return by_law<0>(q, seed, qid, nopp, ndeal, uniform, ways, row);
}

// Parity mode: the MT19937 stream of seed32 walked on the host, the draws four iterations per word through
// mcq_iterations_replay4 (1-5 opponents: its straight forms).  row = 13 words.
int hs_epochs_replay(const mcq_query *q, uint32_t seed32, uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    McqCard base[192];
    memset(base, 0, sizeof(base));
    for (uint32_t l = 0; l < 64; l++) base[128 + l] = mcq_base_entry(qc, l, t.sel8);
    const McqDeckAoS deck = {base};
    const McqSumTabs tabs = mcq_sum_tabs_of(t.tf);
    memset(row, 0, 13 * sizeof(uint64_t));
    row[0] = q->runs;
    const size_t stride = q->runs ? q->runs : 1;
    std::vector<uint8_t> draws((size_t)mcq_draws_per_iteration(*q) * stride + 4);
    row[1] = mcq_replay_parse(*q, seed32, draws.data(), stride);
    for (uint32_t it4 = 0; it4 < q->runs; it4 += 4) {
        McqReplayDraws4 dr;
        dr.load(draws.data() + it4, stride, qc.n_opp, qc.n_deal);
        McqLaneAcc acc = {};
        mcq_iterations_replay4(qc, dr, deck, tabs, acc, q->runs - it4 < 4u ? q->runs - it4 : 4u);
        mcq_tally_fold(acc, row);
    }
    return MCQ_OK;
}
}
