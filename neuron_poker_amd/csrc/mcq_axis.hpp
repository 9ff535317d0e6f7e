// mcq_axis.hpp -- the COST AXIS of the Monte-Carlo kernels: how a batch's wave tasks are shared out among the waves.
// Pure integer arithmetic, written MCQ_HD: mcq_kernels.hip compiles it for gfx950, tests/hostsim_axis for the host.
//
// prefix[0 .. n] is the exclusive prefix of the records' scheduling cost (tasks x weight; prefix[0] = 0, prefix[n] = the
// total); a record that is invalid or has nothing to run costs nothing, so neighbouring entries may be equal.  Record qi
// lies at [prefix[qi], prefix[qi + 1]) and its task t starts at prefix[qi] + t * weight.  The axis is cut into one slice
// per wave, and
//
//     A TASK BELONGS TO THE SLICE ITS START FALLS INTO.
//
// The slices tile [0, total) and every task has one start, so every task is run exactly once, whatever the number of
// waves and wherever the cuts fall inside a task or a record.  A wave therefore begins at the first task of its first
// record that starts at or behind `lo` (mcq_axis_first_task) and ends at the first task that starts at or behind `hi`
// (mcq_axis_owns).
#pragma once
#include "mcq_device.hpp"

struct McqAxisSlice {
    uint64_t lo, hi; /* [lo, hi); lo == hi: nothing (more parts than units) */
};
/* where part i of n_parts of an axis of `total` units begins (total * n_parts < 2^64: the host's grids and prices see
 * to that), and the part itself */
MCQ_HD uint64_t mcq_axis_cut(uint64_t total, uint64_t i, uint64_t n_parts) { return total * i / n_parts; }
MCQ_HD McqAxisSlice mcq_axis_slice(uint64_t total, uint64_t i, uint64_t n_parts) {
    const McqAxisSlice s = {mcq_axis_cut(total, i, n_parts), mcq_axis_cut(total, i + 1ull, n_parts)};
    return s;
}
/* the last record of [0, n) with prefix[i] <= x: the record x lies in when x < total (of equal entries the last one, the
 * one with a positive cost) */
MCQ_HD uint32_t mcq_axis_last_le(const uint64_t *prefix, uint32_t n, uint64_t x) {
    uint32_t a = 0, b = n;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (prefix[mid] <= x) a = mid; else b = mid;
    }
    return a;
}
/* the last record of [from, n) with prefix[i] < x, `from` itself if there is none: the last record that starts before x */
MCQ_HD uint32_t mcq_axis_last_lt(const uint64_t *prefix, uint32_t from, uint32_t n, uint64_t x) {
    uint32_t a = from, b = n;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (prefix[mid] < x) a = mid; else b = mid;
    }
    return a;
}
/* the first task of the record at pfx that starts at or behind lo (not 0 only for the first record of a slice) */
MCQ_HD uint32_t mcq_axis_first_task(uint64_t pfx, uint64_t lo, uint32_t weight) {
    return pfx < lo ? (uint32_t)((lo - pfx + weight - 1) / weight) : 0u;
}
/* does `task` of the record at pfx start before hi, i.e. inside the slice that ends there? */
MCQ_HD bool mcq_axis_owns(uint64_t pfx, uint32_t task, uint32_t weight, uint64_t hi) {
    return pfx + (uint64_t)task * weight < hi;
}
/* the records of a block: those whose cost interval meets the piece of the axis that the block's waves cover (waves
 * block * waves_per_block .. of grid * waves_per_block).  count == 0: the block has no piece. */
struct McqAxisRecords {
    uint32_t first, count;
};
MCQ_HD McqAxisRecords mcq_axis_block_records(const uint64_t *prefix, uint32_t n, uint32_t block, uint32_t waves_per_block,
                                             uint32_t grid) {
    const uint64_t n_waves = (uint64_t)grid * waves_per_block;
    const McqAxisSlice s = {mcq_axis_cut(prefix[n], (uint64_t)block * waves_per_block, n_waves),
                            mcq_axis_cut(prefix[n], (uint64_t)(block + 1u) * waves_per_block, n_waves)};
    McqAxisRecords r = {0u, 0u};
    if (s.lo < s.hi) {
        r.first = mcq_axis_last_le(prefix, n, s.lo);
        r.count = mcq_axis_last_lt(prefix, r.first, n, s.hi) - r.first + 1u;
    }
    return r;
}
