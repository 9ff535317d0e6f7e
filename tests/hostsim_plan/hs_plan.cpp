// hs_plan.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the launch plans (neuron_poker_amd/csrc/mcq_plan.hpp, and mcq_pick_split of mcq_device.hpp): the
// functions the host layer calls before a launch, one by one, their results laid out as words.  hs_rows.hpp adds the
// synthetic weight tables and the row checkers that this file and hs_main.cpp share.
#include "hs_rows.hpp"

extern "C" {
// out: grid, block, split, work_wpb (occ: the same for every mode)
void hs_plan_geometry(uint32_t n_cu, uint32_t occ, uint32_t grid_cap, uint32_t split_max, uint32_t load_waves, int bulk,
                      uint64_t total_tasks, uint64_t max_tasks, uint32_t *out) {
    hs_geometry(n_cu, occ, grid_cap, split_max, load_waves, bulk, total_tasks, max_tasks, out);
}
uint32_t hs_plan_pick_split(uint64_t total_tasks, uint64_t max_tasks, uint32_t n_cu, uint32_t split_max) {
    return mcq_pick_split(total_tasks, max_tasks, n_cu, split_max);
}
// out: lg, grid, rounds
void hs_plan_small_cut(uint64_t n, uint32_t n_cu, uint32_t split_max, uint32_t *out) {
    const McqSmallCut c = mcq_plan_small_cut(n, n_cu, split_max);
    out[0] = c.lg, out[1] = c.grid, out[2] = c.rounds;
}
// out: MCQ_EXT_SMALL_Q, _LISTS, _TASKS, _BLOCKS
void hs_plan_ext_small_limits(uint32_t *out) {
    out[0] = MCQ_EXT_SMALL_Q, out[1] = MCQ_EXT_SMALL_LISTS, out[2] = MCQ_EXT_SMALL_TASKS, out[3] = MCQ_EXT_SMALL_BLOCKS;
}
int hs_plan_ext_small_fits(uint64_t n, uint32_t lists_stride, uint32_t most_tasks) {
    return mcq_ext_small_fits((size_t)n, lists_stride, most_tasks) ? 1 : 0;
}
// a batch that fits -> wpb; blk[MCQ_EXT_SMALL_BLOCKS] unpacked into four words each (query, part, parts, wpb),
// first_block[n + 1], *n_blocks
uint32_t hs_plan_ext_small(const uint32_t *tasks, uint32_t n, uint32_t *blk4, uint32_t *first_block, uint32_t *n_blocks) {
    uint32_t blk[MCQ_EXT_SMALL_BLOCKS];
    const McqExtSmallPlan p = mcq_ext_small_plan(tasks, n, blk);
    for (uint32_t b = 0; b < p.n_blocks; b++) {
        const McqExtSmallBlock u = mcq_ext_small_unpack(blk[b]);
        blk4[4 * b] = u.query, blk4[4 * b + 1] = u.part, blk4[4 * b + 2] = u.parts, blk4[4 * b + 3] = u.wpb;
        if (mcq_ext_small_pack(u) != blk[b]) return 0u;
    }
    for (uint32_t i = 0; i <= n; i++) first_block[i] = p.first_block[i];
    *n_blocks = p.n_blocks;
    return p.wpb;
}
// wc[53]: per card the weight of the hands of w[1326] that hold it, [52] the total
void hs_plan_with_card(const uint16_t *w, uint32_t *wc) { mcq_ranges_with_card(w, wc); }
// tables: n_tables x 1326 weights; q16: the record; seat_row[10] -> out: price, refused, seat, table
void hs_plan_ranges_price(const uint16_t *tables, uint64_t n_tables, const uint8_t *q16, const uint32_t *seat_row, uint32_t *out) {
    hs_price(tables, (size_t)n_tables, q16, seat_row, out);
}
// the synthetic table of hs_rows.hpp (kind, a, b, w) -> w16[1326]
void hs_plan_table(uint32_t kind, uint32_t a, uint32_t b, uint32_t w, uint16_t *w16) { hs_table(kind, a, b, w, w16); }
// out: n_boards, slices, row, grid
void hs_plan_exact(const uint8_t *q16, uint32_t row, uint32_t n_cu, uint32_t *out) {
    mcq_query q;
    memcpy(&q, q16, 16);
    McqExactJob job;
    mcq_exact_plan(&q, row, n_cu, &job);
    out[0] = job.n_boards, out[1] = job.slices, out[2] = job.row, out[3] = job.grid;
    if (memcmp(job.rec, q16, 16) != 0) out[3] = 0xFFFFFFFFu;
}
// out: the return value, then ext, n_boards, row, grid, groups, h1_off
void hs_plan_exact_ext(const uint8_t *q16, uint32_t ext, uint32_t row, uint32_t kind, uint32_t L, uint32_t h1_off, uint32_t n_cu,
                       uint32_t *out) {
    hs_exact_ext(0, q16, ext, row, kind, L, h1_off, n_cu, 0u, out);
}
// (L, n_allowed, slice) -> the same seven words
void hs_plan_exact_hero(int preflop, const uint8_t *q16, uint32_t ext, uint32_t row, uint32_t L, uint32_t n_allowed, uint32_t n_cu,
                        uint32_t slice, uint32_t *out) {
    hs_exact_ext(preflop ? 2 : 1, q16, ext, row, n_allowed, L, 0u, n_cu, slice, out);
}
// a row of plan_rows.inc (kind: 0 geometry, 1 small cut, 2 exact, 3 exact ext / hero, 4 price) -> 1: the header gives its results
int hs_plan_row(uint32_t kind, const uint64_t *v, uint64_t n) {
    switch (kind) {
        case 0: return hs_row_geometry(v, (size_t)n) ? 1 : 0;
        case 1: return hs_row_small_cut(v, (size_t)n) ? 1 : 0;
        case 2: return hs_row_exact(v, (size_t)n) ? 1 : 0;
        case 3: return hs_row_exact_ext(v, (size_t)n) ? 1 : 0;
        case 4: return hs_row_price(v, (size_t)n) ? 1 : 0;
    }
    return 0;
}
}
