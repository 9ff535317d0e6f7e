// hs_stage.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the blocks' staging decisions and the candidate lists' compaction steps
// (neuron_poker_amd/csrc/mcq_stage.hpp): the functions the kernels call, one by one, the serial list of the host builds
// (tests/hostsim/hs_walk.hpp) to hold the compaction against, and the blocks of a whole ranges batch (hs_stage.hpp).
#include "hs_stage.hpp"

#include <string.h>

#include "../hostsim/hs_walk.hpp"

extern "C" {
// MCQ_EXT_STAGE_ENTRIES, MCQ_EXT_STAGE_LISTS, MCQ_RG_STAGE_TABLES, MCQ_RG_STAGE_QUERIES
void hs_stage_consts(uint32_t *out) {
    out[0] = MCQ_EXT_STAGE_ENTRIES;
    out[1] = MCQ_EXT_STAGE_LISTS;
    out[2] = MCQ_RG_STAGE_TABLES;
    out[3] = MCQ_RG_STAGE_QUERIES;
}
// off: MCQ_EXT_STAGE_LISTS + 1 entries
int hs_stage_ext_lists(uint32_t first, uint32_t nq, uint32_t lists_stride, const uint32_t *cnts, uint32_t *off) {
    return mcq_ext_stage_lists(first, nq, lists_stride, cnts, off) ? 1 : 0;
}
uint32_t hs_stage_ranges_slot(const uint32_t *tab_id, uint32_t n_staged, uint32_t t) { return mcq_ranges_stage_slot(tab_id, n_staged, t); }
// the blocks of a batch -> out[9 b ..] = first, count, staged tables, their six ids (0xFFFFFFFF: not written); returns
// the grid, 0 for a batch with a record the host layer refuses; never more than `room` blocks are written
uint32_t hs_stage_ranges_blocks(const mcq_query *q, const uint32_t *seat_table, const uint16_t *tables, uint32_t n_tables, uint32_t n,
                                uint32_t n_cu, uint32_t grid_cap, uint64_t *prefix, uint32_t *out, uint32_t room) {
    const std::vector<hs::RangesBlock> blocks = hs::ranges_blocks(q, seat_table, tables, n_tables, n, n_cu, grid_cap, prefix);
    for (uint32_t b = 0; b < blocks.size() && b < room; b++) {
        out[9u * b] = blocks[b].first;
        out[9u * b + 1u] = blocks[b].count;
        out[9u * b + 2u] = blocks[b].n_staged;
        memcpy(out + 9u * b + 3u, blocks[b].tab_id, sizeof blocks[b].tab_id);
    }
    return (uint32_t)blocks.size();
}
// list li of a valid record: the cards its candidates are made of and its class set (hs::kSetWords words)
void hs_stage_list_plan(const mcq_query *q, const mcq_query_ext *e, uint32_t li, uint64_t *U, uint32_t *set) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    uint32_t set_off;
    mcq_ext_list_plan(mcq_query_words(*q), er, li, *U, set_off);
    memcpy(set, er.w + set_off, hs::kSetWords * sizeof(uint32_t));
}
// per = 11: 256 threads, per = 3: 1024 threads; returns the threads (0: no such instantiation)
uint32_t hs_stage_list_masks(uint32_t per, uint64_t U, const uint32_t *set, uint32_t *masks) {
    if (per == 11u) hs::list_masks<11, 256>(U, set, masks);
    else if (per == 3u) hs::list_masks<3, 1024>(U, set, masks);
    else return 0;
    return per == 11u ? 256u : 1024u;
}
uint32_t hs_stage_list_scatter(uint32_t per, const uint32_t *masks, const uint32_t *at, uint16_t *dst) {
    if (per == 11u) hs::list_scatter<11, 256>(masks, at, dst);
    else if (per == 3u) hs::list_scatter<3, 1024>(masks, at, dst);
    else return 0;
    return per == 11u ? 256u : 1024u;
}
// the serial lists of a record as the host builds of the lane code lay them out: list li -> dst (MCQ_EXT_LIST_STRIDE
// entries of room), returns its length; 0xFFFFFFFF: the record is invalid or has no such list
uint32_t hs_stage_serial_list(const mcq_query *q, const mcq_query_ext *e, uint32_t li, uint16_t *dst) {
    hs::ExtQuery x(q, e);
    if (!x.valid || li >= mcq_ext_n_lists(x.qw, x.er)) return 0xFFFFFFFFu;
    memcpy(dst, x.wc.list[li], x.wc.cnt[li] * sizeof(uint16_t));
    return x.wc.cnt[li];
}
}
