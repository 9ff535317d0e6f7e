// hs_walk.hpp -- TEST HARNESS ONLY (included by the host builds under tests/hostsim*/, never by the product).
//
// What the host builds of the lane code share, so that a shim names only what is its own -- the instantiation it runs and
// the switch it adds -- and every shim walks a query the same way:
//   luts        the filled tables
//   BaseDeck    a query's context and its base deck behind McqDeckAoS
//   streams     one stream of MCQ_STREAM_ITERS iterations per lane, as mcq_eval_kernel walks a query; passes counted HERE
//   replay      parity mode: the host's parse of the MT19937 stream, four iterations per load of every draw row
//   forms       run-time (law, row kind, opponents, cards to come) -> the named instantiation, by a set of forms
//   plans       run-time (rule, plan size) -> template arguments, and explicit draws through a plan's positions
//   ExtQuery    an extended query's contexts, candidate lists and card table, and its two walks
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_replay.hpp"
#include "../../neuron_poker_amd/csrc/mcq_stage.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace hs {

// ---------------------------------------------------------------------------------------------- tables
inline const McqTables &luts() { /* filled once, by whichever thread comes first */
    static const struct Filled {
        McqTables t;
        Filled() { mcq_fill_tables(&t); }
    } filled;
    return filled.t;
}

// ---------------------------------------------------------------------------------------------- base deck
// The iteration takes the deck pointer biased by -128 entries (draw indices carry r | 0x80): 128 unused entries in front.
struct BaseDeck {
    McqQueryCtx qc;
    McqCard card[192];
    explicit BaseDeck(const mcq_query &q) { /* q is valid */
        mcq_query_ctx(mcq_query_words(q), qc);
        memset(card, 0, sizeof card);
        for (uint32_t l = 0; l < 64; l++) card[128 + l] = mcq_base_entry(qc, l, luts().sel8);
    }
    McqDeckAoS aos() const { return McqDeckAoS{card}; }
};

// ---------------------------------------------------------------------------------------------- rows and streams
template <class Acc>
void start_row(uint64_t *row, uint32_t runs) {
    memset(row, 0, (Acc::kSeats ? MCQ_ROW_WORDS_SEATS : Acc::kWays ? MCQ_ROW_WORDS_WAYS : MCQ_ROW_WORDS_PLAIN) * sizeof(uint64_t));
    row[0] = runs;
}

// lane <-> stream: body(dr, acc, cnt) for every stream of the query, cnt = the iterations the stream has (the last is
// ragged).  Every stream's draws start as a copy of `proto` (state a draw policy carries beside the generator's).
template <class Draws, class Acc, class Body>
void each_stream(uint32_t runs, uint64_t seed, uint64_t qid, Body body, const Draws &proto = Draws()) {
    const uint32_t n_streams = (runs + MCQ_STREAM_ITERS - 1) / MCQ_STREAM_ITERS;
    for (uint32_t s = 0; s < n_streams; s++) {
        Draws dr = proto;
        dr.start(seed, qid, s);
        Acc acc = {};
        const uint64_t left = (uint64_t)runs - (uint64_t)s * MCQ_STREAM_ITERS;
        body(dr, acc, left < MCQ_STREAM_ITERS ? (uint32_t)left : MCQ_STREAM_ITERS);
    }
}
// ... folded into a row of 13 or 22 words: iter(dr, acc, cnt) runs a stream's iterations
template <class Draws, class Acc, class Iter>
void walk_streams(const McqQueryCtx &qc, uint32_t runs, uint64_t seed, uint64_t qid, uint64_t *row, Iter iter,
                  const Draws &proto = Draws()) {
    start_row<Acc>(row, runs);
    each_stream<Draws, Acc>(runs, seed, qid, [&](Draws &dr, Acc &acc, uint32_t cnt) {
        iter(dr, acc, cnt);
        acc.passes = cnt * qc.n_opp; /* MCQ-CTR v5: one attempt per opponent, never re-drawn */
        mcq_tally_fold(acc, row);
    }, proto);
}

// ---------------------------------------------------------------------------------------------- parity mode
// The MT19937 stream of seed32 parsed on the host (passes come from the parse alone), then the draws as the kernel reads
// them: four iterations per 32-bit load of every draw row (McqReplayDraws4).  EACH: every iteration on its own through
// the general form (mcq_iteration); else a load's iterations through mcq_iterations_replay4 and its straight forms.
template <class Acc, bool EACH>
int replay_row(const mcq_query *q, uint32_t seed32, uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = luts();
    const BaseDeck bd(*q);
    const McqSumTabs tabs = mcq_sum_tabs_of(t.tf);
    start_row<Acc>(row, q->runs);
    const size_t stride = q->runs ? q->runs : 1;
    std::vector<uint8_t> draws((size_t)mcq_draws_per_iteration(*q) * stride + 4);
    row[MCQ_RW_PASSES] = mcq_replay_parse(*q, seed32, draws.data(), stride);
    for (uint32_t it4 = 0; it4 < q->runs; it4 += 4) {
        const uint32_t cnt4 = q->runs - it4 < 4u ? q->runs - it4 : 4u;
        McqReplayDraws4 dr;
        dr.load(draws.data() + it4, stride, bd.qc.n_opp, bd.qc.n_deal);
        if (!EACH) {
            Acc acc = {};
            mcq_iterations_replay4(bd.qc, dr, bd.aos(), tabs, acc, cnt4);
            mcq_tally_fold(acc, row);
        } else for (uint32_t k = 0; k < cnt4; k++) {
            dr.sh = 8u * k;
            Acc acc = {};
            mcq_iteration(bd.qc, dr, bd.card, t.tf, t.tops, t.sd, acc);
            mcq_tally_fold(acc, row);
        }
    }
    return MCQ_OK;
}

// ---------------------------------------------------------------------------------------------- forms
// An instantiation of mcq_iteration_sum named by the caller: NOPP, NDEAL = -1: counted at run time.
template <class Draws_, class Acc_, int NOPP, int NDEAL>
struct Form {
    typedef Draws_ Draws;
    typedef Acc_ Acc;
    static constexpr int kNopp = NOPP, kNdeal = NDEAL;
    /* a count the form names must be the query's own.  (A set without NOPP = -1 thereby checks the opponents always.) */
    static bool fits(const McqQueryCtx &qc) {
        return (NOPP < 0 || qc.n_opp == (uint32_t)NOPP) && (NDEAL < 0 || qc.n_deal == (uint32_t)NDEAL);
    }
    /* the query's streams through one(dr, acc), an iteration of this form */
    template <class One>
    static int walk(const McqQueryCtx &qc, uint32_t runs, uint64_t seed, uint64_t qid, uint64_t *row, One one) {
        if (!fits(qc)) return MCQ_EINVAL;
        walk_streams<Draws, Acc>(qc, runs, seed, qid, row, [&](Draws &dr, Acc &acc, uint32_t cnt) {
            for (uint32_t j = 0; j < cnt; j++) one(dr, acc);
        });
        return MCQ_OK;
    }
};
// The forms mcq_iterations_sum instantiates: the opponents counted at run time (GENERAL: a set may leave that one out) or
// 1 to 9 with the table cards to come counted at run time, 1 to 7 opponents also with 5, 2 or 1 to come; either law,
// either row kind.  A lean set (a sanitizer program's) is a struct with the same `has`.
template <bool GENERAL>
struct SumForms {
    static constexpr bool has(bool, bool, int nopp, int ndeal) {
        return ndeal == -1 ? (nopp == -1 ? GENERAL : nopp >= 1 && nopp <= 9) : nopp >= 1 && nopp <= 7 && (ndeal == 5 || ndeal == 2 || ndeal == 1);
    }
};
typedef SumForms<true> AllForms;
typedef SumForms<false> StraightForms;

namespace detail {
typedef std::integer_sequence<int, -1, 1, 2, 3, 4, 5, 6, 7, 8, 9> Opps;
typedef std::integer_sequence<int, -1, 5, 2, 1> Deals;
template <class Set, bool U, bool W, int NOPP, int NDEAL, class F>
bool try_form(int ndeal, F &f, int &rc) {
    if constexpr (Set::has(U, W, NOPP, NDEAL)) {
        if (ndeal != NDEAL) return false;
        rc = f(Form<McqCtrDrawsT<U>, std::conditional_t<W, McqLaneAccWays, McqLaneAcc>, NOPP, NDEAL>());
        return true;
    } else return false;
}
template <class Set, bool U, bool W, int NOPP, class F, int... ND>
bool try_opp(int nopp, int ndeal, F &f, int &rc, std::integer_sequence<int, ND...>) {
    return nopp == NOPP && (try_form<Set, U, W, NOPP, ND>(ndeal, f, rc) || ...);
}
template <class Set, bool U, bool W, class F, int... NO>
int for_law(int nopp, int ndeal, F &f, std::integer_sequence<int, NO...>) {
    int rc = MCQ_EINVAL;
    (void)(try_opp<Set, U, W, NO>(nopp, ndeal, f, rc, Deals()) || ...);
    return rc;
}
}  // namespace detail
// f(Form<...>()) -> its return code, for the form the arguments name; MCQ_EINVAL where Set does not hold it
template <class Set, class F>
int for_form(int uniform, int ways, int nopp, int ndeal, F f) {
    if (uniform) return ways ? detail::for_law<Set, true, true>(nopp, ndeal, f, detail::Opps()) : detail::for_law<Set, true, false>(nopp, ndeal, f, detail::Opps());
    return ways ? detail::for_law<Set, false, true>(nopp, ndeal, f, detail::Opps()) : detail::for_law<Set, false, false>(nopp, ndeal, f, detail::Opps());
}

// ---------------------------------------------------------------------------------------------- plans
typedef std::make_integer_sequence<int, MCQ_PLAN_MAX_DRAWS - 1> AllPlanSizes; /* NS + 2: 2 .. 23 draws */
// f(std::integral_constant<int, RULE>()) for a rule plans are built for, f(std::integral_constant<int, N>()) for a plan
// size in Sizes; MCQ_EINVAL for any other
template <class F>
int for_rule(int rule, F f) {
    switch (rule) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case MCQ_DEAL_FULLREG: return f(std::integral_constant<int, MCQ_DEAL_FULLREG>());
        default: return MCQ_EINVAL;
    }
}
template <class F, int... NS>
int for_plan_size(int n_plan, F f, std::integer_sequence<int, NS...>) {
    int rc = MCQ_EINVAL;
    (void)((n_plan == NS + 2 ? (rc = f(std::integral_constant<int, NS + 2>()), true) : false) || ...);
    return rc;
}
template <int N, int RULE, int PAIRED, int D>
void draw_from(const uint8_t *r, int n, uint32_t (&E)[MCQ_PLAN_REGS], uint8_t *pos) {
    if constexpr (D < N) {
        if (D >= n) return;
        pos[D] = (uint8_t)(mcq_draw_epoch<N, RULE, D, PAIRED>(r[D] | 0x80u, E) - 128u);
        draw_from<N, RULE, PAIRED, D + 1>(r, n, E, pos);
    }
}
// draws[rows][n] (r, unbiased) through the first n draws of the plan (n_plan, rule) -> pos[rows][n], base positions
template <class Sizes, int PAIRED = MCQ_COUNT_PAIRED>
int positions(int n_plan, int rule, int n, const uint8_t *draws, uint64_t rows, uint8_t *pos) {
    return for_rule(rule, [&](auto r) {
        return for_plan_size(n_plan, [&](auto np) -> int {
            constexpr int N = decltype(np)::value, RULE = decltype(r)::value;
            if (n < 1 || n > N) return MCQ_EINVAL;
            for (uint64_t i = 0; i < rows; i++) {
                uint32_t E[MCQ_PLAN_REGS] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL,
                                             MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
                draw_from<N, RULE, PAIRED, 0>(draws + i * (uint64_t)n, n, E, pos + i * (uint64_t)n);
            }
            return MCQ_OK;
        }, Sizes());
    });
}

// ---------------------------------------------------------------------------------------------- extended queries
// What mcq_iteration_ext / mcq_iteration_ext_fast take beside the draws: the contexts, the candidate lists laid out as
// mcq_ext_lists_kernel lays them out, the 64-entry card table.  `valid` false: nothing else is set.
struct ExtQuery {
    const mcq_query *q;
    const mcq_query_ext *e;
    McqExtRec er;
    McqQueryWords qw;
    bool valid, empty_list; /* empty_list: a candidate list without a hand (production mode refuses the query) */
    McqExtCtx qc;
    McqExtWaveCtx wc;
    std::vector<uint16_t> lists;
    McqCard cards[64];
    uint16_t ids[MCQ_MAX_OPP + 1];
    ExtQuery(const ExtQuery &) = delete;
    ExtQuery(const mcq_query *q_, const mcq_query_ext *e_)
        : q(q_), e(e_), er{reinterpret_cast<const uint32_t *>(e_)}, qw(mcq_query_words(*q_)), valid(mcq_query_ext_valid(qw, er)), empty_list(false) {
        if (!valid) return;
        mcq_ext_ctx(qw, er, qc);
        memset(&wc, 0, sizeof wc);
        for (uint32_t h = 0; h < qc.n_hands; h++) wc.hand[h] = mcq_ext_hand(qw, er, h);
        const uint32_t n_lists = mcq_ext_n_lists(qw, er);
        lists.resize((size_t)(n_lists ? n_lists : 1) * MCQ_EXT_LIST_STRIDE);
        for (uint32_t li = 0; li < n_lists; li++) {
            uint64_t U;
            uint32_t set_off, cnt = 0;
            uint16_t *list = lists.data() + (size_t)li * MCQ_EXT_LIST_STRIDE;
            mcq_ext_list_plan(qw, er, li, U, set_off);
            for (uint32_t c = 0; c < 2704u; c++) /* one candidate per "thread", the offsets summed on the way */
                cnt = mcq_ext_list_scatter<1>(mcq_ext_list_mask<1>(U, er.w + set_off, c), c, cnt, list);
            wc.cnt[li] = cnt;
            wc.list[li] = list;
            empty_list = empty_list || cnt == 0;
        }
        for (uint32_t c = 0; c < 64; c++) cards[c] = mcq_card(c < 52 ? c : 0);
    }
    // production mode: one stream of mcq_ext_stream_iters iterations per lane; iter(dr, acc, it) runs iteration `it` and
    // says whether it could be dealt (MCQ_EINVAL at the first that could not)
    template <class Acc, class Iter>
    int walk(uint64_t seed, uint64_t qid, uint64_t *row, Iter iter) {
        start_row<Acc>(row, q->runs);
        const uint32_t s_iters = mcq_ext_stream_iters(qw, er);
        const uint32_t n_streams = (q->runs + s_iters - 1) / s_iters;
        for (uint32_t s = 0; s < n_streams; s++) {
            McqExtCtrDraws dr;
            dr.start(seed, qid, s);
            Acc acc = {};
            for (uint32_t j = 0; j < s_iters; j++) {
                const uint64_t it = (uint64_t)s * s_iters + j;
                if (it >= q->runs) break;
                if (!iter(dr, acc, it)) return MCQ_EINVAL;
            }
            mcq_tally_fold(acc, row);
        }
        return MCQ_OK;
    }
    // parity mode: the MT19937 stream of seed32 parsed on the host, iteration by iteration; MCQ_EINVAL: cannot be dealt
    template <class Acc, class Iter>
    int replay(uint32_t seed32, uint64_t *row, Iter iter) {
        start_row<Acc>(row, q->runs);
        const size_t stride = q->runs ? q->runs : 1;
        std::vector<uint8_t> draws((size_t)mcq_ext_draws_per_iteration(*q, *e) * stride + 1);
        McqMt19937 g;
        g.seed(seed32);
        const uint64_t passes = mcq_replay_parse_ext(*q, *e, g, draws.data(), stride, 1000000u);
        if (passes == ~0ull) return MCQ_EINVAL;
        row[MCQ_RW_PASSES] = passes;
        for (uint32_t it = 0; it < q->runs; it++) {
            McqExtReplayDraws dr = {draws.data() + it, stride};
            Acc acc = {};
            iter(dr, acc, it);
            acc.passes = 0; /* they come from the parse alone */
            mcq_tally_fold(acc, row);
        }
        return MCQ_OK;
    }
};

}  // namespace hs
