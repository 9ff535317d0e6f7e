// hs_main.cpp -- TEST HARNESS ONLY: the rows of plan_rows.inc walked by a program of its own, which the tests build with
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_plan_host.py).  One line per kind of row: how many rows
// there are and how many of them the header (neuron_poker_amd/csrc/mcq_plan.hpp) reproduces.
#include <stdio.h>

#include "hs_rows.hpp"

namespace {
struct Tally {
    const char *name;
    bool (*check)(const uint64_t *, size_t);
    unsigned rows, ok;
};
Tally g_tally[] = {{"geometry", hs_row_geometry, 0, 0}, {"small_cut", hs_row_small_cut, 0, 0}, {"exact", hs_row_exact, 0, 0},
                   {"exact_ext", hs_row_exact_ext, 0, 0}, {"price", hs_row_price, 0, 0}};
void row(int kind, const uint64_t *v, size_t n) {
    g_tally[kind].rows++;
    if (g_tally[kind].check(v, n)) g_tally[kind].ok++;
    else printf("%s row %u differs\n", g_tally[kind].name, g_tally[kind].rows);
}
}  // namespace

#define PLAN_ROW(kind, ...)                       \
    {                                             \
        const uint64_t v_[] = {__VA_ARGS__};      \
        row(kind, v_, sizeof v_ / sizeof v_[0]);  \
    }
#define PLAN_GEOMETRY(...) PLAN_ROW(0, __VA_ARGS__)
#define PLAN_SMALL_CUT(...) PLAN_ROW(1, __VA_ARGS__)
#define PLAN_EXACT(...) PLAN_ROW(2, __VA_ARGS__)
#define PLAN_EXACT_EXT(...) PLAN_ROW(3, __VA_ARGS__)
#define PLAN_PRICE(...) PLAN_ROW(4, __VA_ARGS__)

int main() {
#include "plan_rows.inc"
    int rc = 0;
    for (const Tally &t : g_tally) {
        printf("%s: %u of %u rows\n", t.name, t.ok, t.rows);
        if (t.ok != t.rows || t.rows == 0) rc = 1;
    }
    /* the one-launch extended plan at its fullest: eight queries of 64 tasks fill all 32 block words and no more */
    uint32_t tasks[MCQ_EXT_SMALL_Q], blk[MCQ_EXT_SMALL_BLOCKS];
    for (uint32_t i = 0; i < MCQ_EXT_SMALL_Q; i++) tasks[i] = MCQ_EXT_SMALL_TASKS;
    const McqExtSmallPlan p = mcq_ext_small_plan(tasks, MCQ_EXT_SMALL_Q, blk);
    const McqExtSmallBlock last = mcq_ext_small_unpack(blk[p.n_blocks - 1u]);
    printf("ext_small: wpb %u, blocks %u, last %u %u %u %u\n", p.wpb, p.n_blocks, last.query, last.part, last.parts, last.wpb);
    return rc;
}
