// hs_ext_ways.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the product's EXTENDED lane code with the split-pot switch ON (McqLaneAccWays: mcq_iteration_ext and
// mcq_iteration_ext_fast, neuron_poker_amd/csrc/mcq_device.hpp) for the HOST compiler and walks the kernels' stream / lane
// decomposition sequentially, as tests/hostsim does for the credited form.  The oracle has no per-iteration trace for
// extended queries, so this build also hands back every iteration's dealt hands -- through MCQ_EXT_DEAL_HOOK, which
// exists in host builds only -- and the tests recount the ways from them with the oracle's own comparison.
// The exact enumeration's split-pot lane code (mcq_exact_ext.hpp, kinds 0 and 1) is walked here too.
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
#define MCQ_EXT_DEAL_HOOK(h, c1, c2) hs_dealt(h, c1, c2)

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_ext.hpp"

extern "C" {

// replay != 0: MT19937 replay with seed32 = seed (the caller adds the query id); else MCQ-CTR v5x.  general != 0: every
// iteration through mcq_iteration_ext (else the form the kernels pick: the fast one where it applies).  out: 22 words.
// hands (may be null): runs x (2 n_players + 5) card ids.
int hs_ext_ways_run(int replay, const mcq_query *q, const mcq_query_ext *e, uint64_t seed, uint64_t qid, int general,
                    mcq_result_ways *out, uint8_t *hands) {
    hs::ExtQuery x(q, e);
    if (!x.valid || (x.empty_list && !replay)) return MCQ_EINVAL;
    const McqTables &t = hs::luts();
    uint64_t *row = reinterpret_cast<uint64_t *>(out);
    const uint32_t rec = 2u * q->n_players + 5u;
    g_players = q->n_players;
    g_board = q->n_board;
    struct Unhook { ~Unhook() { g_hands = nullptr; } } unhook;
    auto begin = [&](uint64_t it) {
        if (!hands) return;
        g_hands = hands + it * rec;
        g_hands[0] = q->hole[0]; /* (the fast form never deals hero: its hand is part of the query) */
        g_hands[1] = q->hole[1];
        for (uint32_t k = 0; k < q->n_board; k++) g_hands[2u * q->n_players + k] = q->board[k];
    };
    if (replay)
        return x.replay<McqLaneAccWays>((uint32_t)seed, row, [&](McqExtReplayDraws &dr, McqLaneAccWays &acc, uint64_t it) {
            begin(it);
            mcq_iteration_ext<McqExtReplayDraws, false, McqLaneAccWays>(x.qc, x.wc, dr, x.cards, t.sel8, x.ids, 1, t.tf, t.tops, t.sd, acc);
        });
    return x.walk<McqLaneAccWays>(seed, qid, row, [&](McqExtCtrDraws &dr, McqLaneAccWays &acc, uint64_t it) {
        begin(it);
        return x.qc.fast && !general
            ? mcq_iteration_ext_fast<McqExtCtrDraws, true, false, McqLaneAccWays>(x.qc, x.wc, dr, x.cards, t.sel8, t.tf, t.tops, t.sd, acc)
            : mcq_iteration_ext<McqExtCtrDraws, false, McqLaneAccWays>(x.qc, x.wc, dr, x.cards, t.sel8, x.ids, 1, t.tf, t.tops, t.sd, acc);
    });
}

// 1 if the kernels take the fast form for this query
int hs_ext_ways_is_fast(const mcq_query *q, const mcq_query_ext *e) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    McqExtCtx qc;
    mcq_ext_ctx(mcq_query_words(*q), er, qc);
    return qc.fast ? 1 : 0;
}

// What the host layer and the kernels cut a batch by (tests/test_ext_kernel_grid_gpu.py mirrors their choice of path, of
// the waves per block and of the lists' placement): candidate lists, iterations per stream, wave tasks and the cost of
// one, and the length of list li as mcq_ext_lists_kernel lays it out (0 for a list the query does not have).
uint32_t hs_ext_n_lists(const mcq_query *q, const mcq_query_ext *e) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    return mcq_ext_n_lists(mcq_query_words(*q), er);
}
uint32_t hs_ext_stream_iters(const mcq_query *q, const mcq_query_ext *e) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    return mcq_ext_stream_iters(mcq_query_words(*q), er);
}
uint32_t hs_ext_task_count(const mcq_query *q, const mcq_query_ext *e) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    const McqQueryWords qw = mcq_query_words(*q);
    return mcq_ext_task_count(qw, mcq_ext_stream_iters(qw, er));
}
uint32_t hs_ext_task_weight(const mcq_query *q, const mcq_query_ext *e) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    const McqQueryWords qw = mcq_query_words(*q);
    return mcq_ext_task_weight(qw, mcq_ext_stream_iters(qw, er));
}
uint32_t hs_ext_list_len(const mcq_query *q, const mcq_query_ext *e, uint32_t li) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    const McqQueryWords qw = mcq_query_words(*q);
    if (li >= mcq_ext_n_lists(qw, er)) return 0;
    uint64_t U;
    uint32_t set_off, cnt = 0;
    mcq_ext_list_plan(qw, er, li, U, set_off);
    for (uint32_t c = 0; c < 2704u; c++) cnt += mcq_ext_candidate(U, er.w + set_off, c) ? 1u : 0u;
    return cnt;
}

// The exact enumeration's split-pot lane code, kinds 0 and 1, walked as mcq_exact_ext_kernel<KIND, true> walks it.
// -> 0, MCQ_XX_* (1..4), 5 = cannot be dealt, 6 = two random opponents.  weights: 22 words.
int hs_exact_ext_ways(const mcq_query *q, const mcq_query_ext *x, int law, uint64_t *weights) {
    const McqTables &t = hs::luts();
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    const int why = mcq_exact_ext_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e, r_id);
    if (!mcq_exact_ext_dealable(e, r_id)) return 5;
    if (e.b.n_opp == 2u) return 6;
    std::vector<uint8_t> cb_tab(MCQ_XX_MAX_RP);
    mcq_exact_ext_cb_table(e, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> pair_xy(MCQ_EXACT_PAIRS);
    for (uint32_t i = 0; i < MCQ_EXACT_PAIRS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    mcq_result_ways w;
    memset(&w, 0, sizeof w);
    const uint32_t n_boards = mcq_exact_binom(e.b.L, e.b.k);
    for (uint32_t board = 0; board < n_boards; board++) {
        uint32_t type, n_eq;
        if (e.b.n_opp == 0u) {
            McqExactAcc acc = {0, 0, 0};
            type = mcq_exact_ext_lone_ways(e, board, t.sel8, t.tf, t.tops, t.sd, acc, n_eq);
            w.r.runs += acc.tot; w.r.win += acc.win; w.r.tie += acc.tie;
            w.r.by_type[type] += acc.win + acc.tie;
            if (acc.tie) w.tie_ways[n_eq - 1u] += acc.tie;
            continue;
        }
        uint32_t pos[5];
        mcq_exact_unrank(board, e.b.L, e.b.k, pos);
        McqExactBoard bd;
        mcq_exact_board(e.b, pos, t.sel8, t.tf, t.tops, t.sd, bd);
        type = mcq_key_type(bd.hero_key);
        const uint32_t kb = mcq_exact_ext_known_best_eq(e, bd, t.tf, t.tops, t.sd, n_eq);
        McqCard rem_card[64];
        uint32_t rem_pos[64];
        for (uint32_t l = 0; l < e.m; l++) {
            rem_pos[l] = mcq_exact_rem_pos(pos, l);
            rem_card[l] = mcq_card(r_id[rem_pos[l]]);
        }
        McqExactAccWays acc = {0, 0, 0, 0};
        for (uint32_t lane = 0; lane < 64; lane++)
            mcq_exact_ext_pass_a(e, bd, kb, lane, 64u, pair_xy.data(), rem_card, rem_pos, cb_tab.data(), t.tf, t.tops, t.sd,
                                 (uint32_t *)nullptr, (uint32_t *)nullptr, acc);
        w.r.runs += acc.tot; w.r.win += acc.win; w.r.tie += acc.tie;
        w.r.by_type[type] += acc.win + acc.tie;
        w.tie_ways[n_eq] += acc.tie_c;
        if (acc.tie != acc.tie_c) w.tie_ways[n_eq - 1u] += acc.tie - acc.tie_c;
    }
    memcpy(weights, &w, sizeof w);
    return 0;
}
}
