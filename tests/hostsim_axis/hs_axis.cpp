// hs_axis.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the cost-axis arithmetic (neuron_poker_amd/csrc/mcq_axis.hpp): the functions the evaluation kernels call,
// one by one, and a walk of every wave's slice made of nothing but them (first record, first task, task after task, record
// after record, up to the first task that starts behind the slice).  The walk is this file's own: it checks that the
// arithmetic hands every task out once, not the kernels' loops around it (their `fresh` state, tally flushes and failure
// marker), which the GPU tests cover.
#include <stdint.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_axis.hpp"

namespace {
// the (record, task) pairs that wave `wave` of n_waves runs; tasks[i] == 0: a record without cost
template <class Emit>
void walk(const uint64_t *prefix, const uint32_t *tasks, const uint32_t *weight, uint32_t n, uint32_t wave, uint32_t n_waves, Emit emit) {
    const McqAxisSlice slice = mcq_axis_slice(prefix[n], wave, n_waves);
    if (slice.lo >= slice.hi) return;
    for (uint32_t qi = mcq_axis_last_le(prefix, n, slice.lo); qi < n; qi++) {
        const uint64_t pfx = prefix[qi];
        const uint32_t n_tasks = prefix[qi + 1] > pfx ? tasks[qi] : 0u;
        for (uint32_t task = mcq_axis_first_task(pfx, slice.lo, weight[qi]); task < n_tasks; task++) {
            if (!mcq_axis_owns(pfx, task, weight[qi], slice.hi)) return;
            emit(qi, task);
        }
    }
}
}  // namespace

extern "C" {
void hs_axis_slice(uint64_t total, uint64_t i, uint64_t n_parts, uint64_t *lo_hi) {
    const McqAxisSlice s = mcq_axis_slice(total, i, n_parts);
    lo_hi[0] = s.lo;
    lo_hi[1] = s.hi;
}
uint32_t hs_axis_last_le(const uint64_t *prefix, uint32_t n, uint64_t x) { return mcq_axis_last_le(prefix, n, x); }
uint32_t hs_axis_last_lt(const uint64_t *prefix, uint32_t from, uint32_t n, uint64_t x) { return mcq_axis_last_lt(prefix, from, n, x); }
uint32_t hs_axis_first_task(uint64_t pfx, uint64_t lo, uint32_t weight) { return mcq_axis_first_task(pfx, lo, weight); }
int hs_axis_owns(uint64_t pfx, uint32_t task, uint32_t weight, uint64_t hi) { return mcq_axis_owns(pfx, task, weight, hi) ? 1 : 0; }
void hs_axis_block_records(const uint64_t *prefix, uint32_t n, uint32_t block, uint32_t waves_per_block, uint32_t grid, uint32_t *first_count) {
    const McqAxisRecords r = mcq_axis_block_records(prefix, n, block, waves_per_block, grid);
    first_count[0] = r.first;
    first_count[1] = r.count;
}
// the pairs of one wave: out[2 k] = record, out[2 k + 1] = task; returns their number (never more than `room` are written)
uint64_t hs_axis_walk(const uint64_t *prefix, const uint32_t *tasks, const uint32_t *weight, uint32_t n, uint32_t wave, uint32_t n_waves,
                      uint32_t *out, uint64_t room) {
    uint64_t k = 0;
    walk(prefix, tasks, weight, n, wave, n_waves, [&](uint32_t qi, uint32_t task) {
        if (k < room) {
            out[2 * k] = qi;
            out[2 * k + 1] = task;
        }
        k++;
    });
    return k;
}
// Every batch of 1..max_n records with 0..max_tasks tasks each at one of the given weights, cut for 1..max_waves waves:
// how often each task of each record was run, over all the waves.  Returns the number of (batch, n_waves) cases in which
// some task was not run exactly once or something else was run; *cases = how many were looked at, bad[0..4) = the first
// such case (n, n_waves, its index among the batches of n records, the record).
uint64_t hs_axis_partition_exhaustive(uint32_t max_n, uint32_t max_tasks, const uint32_t *weights, uint32_t n_weights, uint32_t max_waves,
                                      uint64_t *cases, uint32_t *bad) {
    uint64_t n_bad = 0;
    *cases = 0;
    const uint32_t per = (max_tasks + 1u) * n_weights; /* choices per record */
    for (uint32_t n = 1; n <= max_n; n++) {
        uint64_t batches = 1;
        for (uint32_t i = 0; i < n; i++) batches *= per;
        std::vector<uint64_t> prefix(n + 1);
        std::vector<uint32_t> tasks(n), weight(n), seen;
        for (uint64_t b = 0; b < batches; b++) {
            uint64_t c = b;
            prefix[0] = 0;
            for (uint32_t i = 0; i < n; i++, c /= per) {
                tasks[i] = (uint32_t)(c % per) / n_weights;
                weight[i] = weights[(c % per) % n_weights];
                prefix[i + 1] = prefix[i] + (uint64_t)tasks[i] * weight[i];
            }
            for (uint32_t n_waves = 1; n_waves <= max_waves; n_waves++) {
                seen.assign((size_t)n * (max_tasks + 1u), 0u);
                bool ok = true;
                for (uint32_t w = 0; w < n_waves; w++)
                    walk(prefix.data(), tasks.data(), weight.data(), n, w, n_waves, [&](uint32_t qi, uint32_t task) {
                        if (qi >= n || task >= tasks[qi]) ok = false;
                        else seen[(size_t)qi * (max_tasks + 1u) + task]++;
                    });
                uint32_t where = 0;
                for (uint32_t i = 0; i < n; i++)
                    for (uint32_t t = 0; t <= max_tasks; t++)
                        if (seen[(size_t)i * (max_tasks + 1u) + t] != (t < tasks[i] ? 1u : 0u)) {
                            ok = false;
                            where = i;
                        }
                (*cases)++;
                if (!ok && n_bad++ == 0) {
                    bad[0] = n;
                    bad[1] = n_waves;
                    bad[2] = (uint32_t)b;
                    bad[3] = where;
                }
            }
        }
    }
    return n_bad;
}
}
