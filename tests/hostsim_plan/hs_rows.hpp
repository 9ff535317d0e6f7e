// hs_rows.hpp -- TEST HARNESS ONLY: what hs_plan.cpp (the library the tests load) and hs_main.cpp (the stand-alone program
// under the host sanitizers) share: the calls into neuron_poker_amd/csrc/mcq_plan.hpp with their results laid out as
// words, the synthetic weight tables of the price rows, and one checker per kind of row of plan_rows.inc.  A row is a
// list of integers, results first: the checker recomputes the results from the rest.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_plan.hpp"

// out: grid, block, split, work_wpb (occ: the same for every mode)
static inline void hs_geometry(uint32_t n_cu, uint32_t occ, uint32_t grid_cap, uint32_t split_max, uint32_t load_waves, int bulk,
                               uint64_t total_tasks, uint64_t max_tasks, uint32_t *out) {
    McqPlanKnobs k;
    k.n_cu = n_cu;
    k.occ[0] = k.occ[1] = k.occ[2] = occ;
    k.grid_cap = grid_cap, k.split_max = split_max, k.load_waves = load_waves;
    const McqGeometry g = mcq_plan_geometry(k, MCQ_MODE_PHILOX, total_tasks, bulk != 0, max_tasks);
    out[0] = g.grid, out[1] = g.block, out[2] = g.split, out[3] = g.work_wpb;
}
// out: price, refused, seat, table
static inline void hs_price(const uint16_t *tables, size_t n_tables, const uint8_t *q16, const uint32_t *seat_row, uint32_t *out) {
    std::vector<uint32_t> wc(n_tables * MCQ_RG_WITH_CARD_STRIDE);
    for (size_t t = 0; t < n_tables; t++) mcq_ranges_with_card(tables + t * MCQ_HAND_ROWS, wc.data() + t * MCQ_RG_WITH_CARD_STRIDE);
    McqQueryWords qw;
    memcpy(&qw, q16, 16);
    const McqRangesPrice p = mcq_ranges_price(tables, n_tables, wc.data(), qw, seat_row);
    out[0] = p.price, out[1] = p.refused, out[2] = p.seat, out[3] = p.table;
}
// which 0: mcq_exact_ext_plan(kind = x, L, h1_off); 1 / 2: mcq_exact_hero_plan postflop / preflop (n_allowed = x, L, slice)
// out: the return value, then ext, n_boards, row, grid, groups, h1_off of the job
static inline void hs_exact_ext(int which, const uint8_t *q16, uint32_t ext, uint32_t row, uint32_t x, uint32_t L, uint32_t h1_off,
                                uint32_t n_cu, uint32_t slice, uint32_t *out) {
    mcq_query q;
    memcpy(&q, q16, 16);
    McqExactExtJob job;
    memset(&job, 0xEE, sizeof job);
    out[0] = which == 0 ? mcq_exact_ext_plan(&q, ext, row, x, L, h1_off, n_cu, &job)
                        : mcq_exact_hero_plan(which == 2, &q, ext, row, L, x, n_cu, slice, &job);
    out[1] = job.ext, out[2] = job.n_boards, out[3] = job.row, out[4] = job.grid, out[5] = job.groups, out[6] = job.h1_off;
    if (memcmp(job.rec, q16, 16) != 0) out[0] = 0xFFFFFFFFu;
}
// a record with the first cards of `board` on the table
static inline void hs_query(uint32_t n_board, const uint64_t *board, uint32_t n_players, uint32_t runs, uint8_t *q16) {
    mcq_query q;
    memset(&q, 0, sizeof q);
    q.hole[0] = 255, q.hole[1] = 255;
    for (uint32_t i = 0; i < 5u; i++) q.board[i] = i < n_board ? (uint8_t)board[i] : 255;
    q.n_board = (uint8_t)n_board, q.n_players = (uint8_t)n_players, q.runs = runs;
    memcpy(q16, &q, 16);
}
// The synthetic weight tables of the price rows (tests/test_plan_host.py builds the same ones in numpy):
//   kind 0  every hand at weight w                         kind 1  the one hand {a, b} at weight w (a known hand)
//   kind 2  hand number i at weight 1 + i % w where i % a == b, the others 0
//   kind 3  the 51 hands that hold card a at weight w      kind 4  nothing (every weight 0)
static inline void hs_table(uint32_t kind, uint32_t a, uint32_t b, uint32_t w, uint16_t *w16) {
    for (uint32_t hi = 1; hi < 52u; hi++)
        for (uint32_t lo = 0; lo < hi; lo++) {
            const uint32_t i = MCQ_HAND_INDEX(lo, hi);
            uint32_t v = 0;
            if (kind == 0u) v = w;
            else if (kind == 1u) v = (lo == (a < b ? a : b) && hi == (a < b ? b : a)) ? w : 0u;
            else if (kind == 2u) v = i % a == b ? 1u + i % w : 0u;
            else if (kind == 3u) v = (lo == a || hi == a) ? w : 0u;
            w16[i] = (uint16_t)v;
        }
}

// ---- the rows (plan_rows.inc): results first; true = the header gives these results
static inline bool hs_same(const uint32_t *got, const uint64_t *want, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (got[i] != want[i]) return false;
    return true;
}
// grid, block, split, work_wpb | n_cu, occ, grid_cap, split_max, load_waves, bulk, total_tasks, max_tasks
static inline bool hs_row_geometry(const uint64_t *v, size_t n) {
    uint32_t out[4];
    if (n != 12) return false;
    hs_geometry((uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint32_t)v[7], (uint32_t)v[8], (int)v[9], v[10], v[11], out);
    return hs_same(out, v, 4);
}
// lg, grid, rounds | n, n_cu, split_max
static inline bool hs_row_small_cut(const uint64_t *v, size_t n) {
    if (n != 6) return false;
    const McqSmallCut c = mcq_plan_small_cut(v[3], (uint32_t)v[4], (uint32_t)v[5]);
    const uint32_t out[3] = {c.lg, c.grid, c.rounds};
    return hs_same(out, v, 3);
}
// n_boards, slices, grid | n_board, n_players, n_cu
static inline bool hs_row_exact(const uint64_t *v, size_t n) {
    if (n != 6) return false;
    const uint64_t board[5] = {0, 1, 2, 3, 4};
    uint8_t q16[16];
    hs_query((uint32_t)v[3], board, (uint32_t)v[4], 1u, q16);
    mcq_query q;
    memcpy(&q, q16, 16);
    McqExactJob job;
    mcq_exact_plan(&q, 7u, (uint32_t)v[5], &job);
    const uint32_t out[3] = {job.n_boards, job.slices, job.grid};
    return hs_same(out, v, 3) && job.row == 7u && memcmp(job.rec, q16, 16) == 0;
}
// returned, n_boards, grid, groups | which (0: x = kind; 1, 2: x = n_allowed, post- and preflop), n_board, x, L, n_cu, slice
static inline bool hs_row_exact_ext(const uint64_t *v, size_t n) {
    if (n != 10) return false;
    const uint64_t board[5] = {0, 1, 2, 3, 4};
    uint8_t q16[16];
    hs_query((uint32_t)v[5], board, 2u, 1u, q16);
    uint32_t o[7];
    hs_exact_ext((int)v[4], q16, 5u, 6u, (uint32_t)v[6], (uint32_t)v[7], v[4] == 0 ? 24u : 0u, (uint32_t)v[8], (uint32_t)v[9], o);
    const uint32_t out[4] = {o[0], o[2], o[4], o[5]};
    return hs_same(out, v, 4) && o[1] == 5u && o[3] == 6u && o[6] == (v[4] == 0 ? 24u : 0u);
}
// price, refused, seat, table | n_board, five table cards, n_players, n_tables, the seats' table numbers (n_players),
// then kind, a, b, w per table
static inline bool hs_row_price(const uint64_t *v, size_t n) {
    if (n < 12) return false;
    const uint32_t n_board = (uint32_t)v[4], n_players = (uint32_t)v[10], n_tables = (uint32_t)v[11];
    if (n_players > 10u || n != 12u + n_players + 4u * (size_t)n_tables) return false;
    uint8_t q16[16];
    hs_query(n_board, v + 5, n_players, 1000u, q16);
    uint32_t seat_row[10] = {0};
    for (uint32_t s = 0; s < n_players; s++) seat_row[s] = (uint32_t)v[12 + s];
    std::vector<uint16_t> tables((size_t)n_tables * MCQ_HAND_ROWS);
    const uint64_t *t = v + 12 + n_players;
    for (uint32_t k = 0; k < n_tables; k++)
        hs_table((uint32_t)t[4 * k], (uint32_t)t[4 * k + 1], (uint32_t)t[4 * k + 2], (uint32_t)t[4 * k + 3], tables.data() + (size_t)k * MCQ_HAND_ROWS);
    uint32_t out[4];
    hs_price(tables.data(), n_tables, q16, seat_row, out);
    return hs_same(out, v, 4);
}
