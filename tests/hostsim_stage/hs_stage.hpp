// hs_stage.hpp -- TEST HARNESS ONLY (built by tests/, never by the product).
//
// Host build of what a block decides before its waves start (neuron_poker_amd/csrc/mcq_stage.hpp), shared by the library
// tests/hostsim_stage loads and the program the tests run under the sanitizers:
//   compaction   the candidate lists' two per-thread steps as a block of THREADS threads takes them, a serial exclusive
//                sum of the threads' counts in between
//   ranges       a batch's cost prefix (mcq_ranges_price, mcq_ranges_task_weight), its grid (mcq_plan_geometry), every
//                block's records (mcq_axis_block_records) and what the block stages
#pragma once
#include <stdint.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_plan.hpp"
#include "../../neuron_poker_amd/csrc/mcq_stage.hpp"

namespace hs {
constexpr uint32_t kSetWords = 6; /* a class set: 169 bits */

// the two instantiations the kernels have: PER candidates per thread x THREADS threads
template <uint32_t PER, uint32_t THREADS>
void list_masks(uint64_t U, const uint32_t *set, uint32_t *masks) {
    static_assert(PER * THREADS >= 2704u, "every candidate has a thread");
    for (uint32_t t = 0; t < THREADS; t++) masks[t] = mcq_ext_list_mask<PER>(U, set, t);
}
/* at[t] = the survivors of the threads below t; thread t writes behind dst[at[t]] */
template <uint32_t PER, uint32_t THREADS>
void list_scatter(const uint32_t *masks, const uint32_t *at, uint16_t *dst) {
    for (uint32_t t = 0; t < THREADS; t++) mcq_ext_list_scatter<PER>(masks[t], t, at[t], dst);
}
template <uint32_t PER, uint32_t THREADS>
std::vector<uint16_t> compact(uint64_t U, const uint32_t *set) {
    std::vector<uint32_t> masks(THREADS), at(THREADS);
    list_masks<PER, THREADS>(U, set, masks.data());
    uint32_t total = 0;
    for (uint32_t t = 0; t < THREADS; t++) {
        at[t] = total;
        total += mcq_popc(masks[t]);
    }
    std::vector<uint16_t> list(total); /* exactly its length: a write beyond it is out of bounds */
    list_scatter<PER, THREADS>(masks.data(), at.data(), list.data());
    return list;
}

// One block of a ranges batch: its records and the tables it stages (n_staged = 0: none).
struct RangesBlock {
    uint32_t first, count, n_staged, tab_id[MCQ_RG_STAGE_TABLES];
};
// The blocks of a batch of n valid records (seat_table: MCQ_MAX_SEATS entries per record) on n_cu compute units with at
// most grid_cap blocks (0: no cap), as mcq_eval_batch_ranges launches mcq_eval_ranges_kernel.  prefix: n + 1 entries out.
inline std::vector<RangesBlock> ranges_blocks(const mcq_query *q, const uint32_t *seat_table, const uint16_t *tables, uint32_t n_tables,
                                              uint32_t n, uint32_t n_cu, uint32_t grid_cap, uint64_t *prefix) {
    std::vector<uint32_t> with_card((size_t)n_tables * MCQ_RG_WITH_CARD_STRIDE), cum((size_t)n_tables * MCQ_RG_CUM_STRIDE, 0u);
    for (uint32_t t = 0; t < n_tables; t++) {
        mcq_ranges_with_card(tables + (size_t)t * MCQ_HAND_ROWS, with_card.data() + (size_t)t * MCQ_RG_WITH_CARD_STRIDE);
        mcq_ranges_prefix(tables + (size_t)t * MCQ_HAND_ROWS, cum.data() + (size_t)t * MCQ_RG_CUM_STRIDE);
    }
    uint64_t total_tasks = 0;
    prefix[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        const McqQueryWords qw = mcq_query_words(q[i]);
        const McqRangesPrice pr = mcq_ranges_price(tables, n_tables, with_card.data(), qw, seat_table + (size_t)i * MCQ_MAX_SEATS);
        if (!mcq_ranges_query_valid(qw) || pr.refused) return {};
        prefix[i + 1] = prefix[i] + (uint64_t)mcq_ranges_task_count(qw) * (mcq_ranges_task_weight(qw) * pr.price);
        total_tasks += mcq_ranges_task_count(qw);
    }
    McqPlanKnobs knobs;
    knobs.n_cu = n_cu;
    knobs.grid_cap = grid_cap;
    const McqGeometry geo = mcq_plan_geometry(knobs, MCQ_MODE_PHILOX, total_tasks);
    std::vector<RangesBlock> blocks(geo.grid);
    for (uint32_t b = 0; b < geo.grid; b++) {
        const McqAxisRecords mine = mcq_axis_block_records(prefix, n, b, geo.block / 64u, geo.grid);
        RangesBlock &r = blocks[b];
        r.first = mine.first;
        r.count = mine.count;
        for (uint32_t k = 0; k < MCQ_RG_STAGE_TABLES; k++) r.tab_id[k] = 0xFFFFFFFFu;
        r.n_staged = mcq_ranges_stage_tables(reinterpret_cast<const uint32_t *>(q), seat_table, cum.data(), mine.first, mine.count, r.tab_id);
    }
    return blocks;
}
}  // namespace hs
