// hs_ways.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the product's lane code with the split-pot switch ON (McqLaneAccWays: neuron_poker_amd/csrc/mcq_device.hpp)
// for the HOST compiler and walks the kernels' task / lane decomposition sequentially, as tests/hostsim does for the
// plain form, so that the 22-word rows of mcq_result_ways can be pinned to the oracle's per-iteration trace in a
// container that has no GPU.  The lanes are folded as WaveTallyWays folds them: `tie` is the sum of the ways.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_replay.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace {
McqTables g_tab;
bool g_init = false;
const McqTables &luts() {
    if (!g_init) { mcq_fill_tables(&g_tab); g_init = true; }
    return g_tab;
}
void make_base(const McqQueryCtx &qc, const McqTables &t, McqCard *store) {
    for (uint32_t l = 0; l < 64; l++) store[128 + l] = mcq_base_entry(qc, l, t.sel8);
}

template <class Draws, bool STRAIGHT>
int run_ctr_t(const mcq_query *q, uint64_t seed, uint64_t qid, mcq_result_ways *out) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    static thread_local McqCard base[192];
    make_base(qc, t, base);
    memset(out, 0, sizeof(*out));
    out->r.runs = q->runs;
    const uint32_t n_streams = (q->runs + MCQ_STREAM_ITERS - 1) / MCQ_STREAM_ITERS;
    for (uint32_t s = 0; s < n_streams; s++) {
        Draws dr;
        dr.start(seed, qid, s);
        McqLaneAccWays acc = {};
        const uint64_t left = (uint64_t)q->runs - (uint64_t)s * MCQ_STREAM_ITERS;
        const uint32_t cnt = left < MCQ_STREAM_ITERS ? (uint32_t)left : MCQ_STREAM_ITERS;
        if (STRAIGHT) mcq_iterations<true>(qc, dr, base, t.tf, t.tops, t.sd, acc, cnt); /* as the bulk kernel runs them */
        else for (uint32_t j = 0; j < cnt; j++) mcq_iteration(qc, dr, base, t.tf, t.tops, t.sd, acc); /* the one-launch kernel */
        acc.passes += cnt * qc.n_opp;
        mcq_tally_fold(acc, reinterpret_cast<uint64_t *>(out));
    }
    return MCQ_OK;
}
}  // namespace

extern "C" {

// mode: 0 = MT19937 replay (seed32 = seed + qid), 1 = MCQ-CTR, 2 = MCQ-CTR under the uniform law (oracle.MODE_*);
// general != 0: every iteration through the general form of mcq_iteration.  out: 22 words.
int hs_ways_run(int mode, const mcq_query *q, uint64_t seed, uint64_t qid, int general, mcq_result_ways *out) {
    if (mode == 1) return general ? run_ctr_t<McqCtrDraws, false>(q, seed, qid, out) : run_ctr_t<McqCtrDraws, true>(q, seed, qid, out);
    if (mode == 2)
        return general ? run_ctr_t<McqCtrDrawsUniform, false>(q, seed, qid, out) : run_ctr_t<McqCtrDrawsUniform, true>(q, seed, qid, out);
    if (mode != 0) return MCQ_EINVAL;
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = luts();
    McqQueryCtx qc;
    mcq_query_ctx(mcq_query_words(*q), qc);
    static thread_local McqCard base[192];
    make_base(qc, t, base);
    memset(out, 0, sizeof(*out));
    out->r.runs = q->runs;
    const size_t stride = q->runs ? q->runs : 1;
    std::vector<uint8_t> draws((size_t)mcq_draws_per_iteration(*q) * stride + 4);
    out->r.passes = mcq_replay_parse(*q, (uint32_t)(seed + qid), draws.data(), stride);
    for (uint32_t it4 = 0; it4 < q->runs; it4 += 4) { /* four iterations per load of every draw row, as the kernel */
        McqReplayDraws4 dr;
        dr.load(draws.data() + it4, stride, qc.n_opp, qc.n_deal);
        for (uint32_t k = 0; k < 4 && it4 + k < q->runs; k++) {
            dr.sh = 8u * k;
            McqLaneAccWays acc = {};
            mcq_iteration(qc, dr, base, t.tf, t.tops, t.sd, acc);
            acc.passes = 0;
            mcq_tally_fold(acc, reinterpret_cast<uint64_t *>(out));
        }
    }
    return MCQ_OK;
}

uint32_t hs_ways_row_bytes(void) { return (uint32_t)sizeof(mcq_result_ways); }
}
