// hs_ways.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the product's lane code with the split-pot switch ON (McqLaneAccWays: neuron_poker_amd/csrc/mcq_device.hpp)
// for the HOST compiler and walks the kernels' task / lane decomposition sequentially, as tests/hostsim does for the
// plain form, so that the 22-word rows of mcq_result_ways can be pinned to the oracle's per-iteration trace in a
// container that has no GPU.  The lanes are folded as WaveTallyWays folds them: `tie` is the sum of the ways.
#include "../hostsim/hs_walk.hpp"

namespace {
template <class Draws, bool STRAIGHT>
int run_ctr_t(const mcq_query *q, uint64_t seed, uint64_t qid, mcq_result_ways *out) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    const McqTables &t = hs::luts();
    const hs::BaseDeck bd(*q);
    hs::walk_streams<Draws, McqLaneAccWays>(bd.qc, q->runs, seed, qid, reinterpret_cast<uint64_t *>(out), [&](Draws &dr, McqLaneAccWays &acc, uint32_t cnt) {
        if (STRAIGHT) mcq_iterations<true>(bd.qc, dr, bd.card, t.tf, t.tops, t.sd, acc, cnt); /* as the bulk kernel runs them */
        else for (uint32_t j = 0; j < cnt; j++) mcq_iteration(bd.qc, dr, bd.card, t.tf, t.tops, t.sd, acc); /* the one-launch kernel */
    });
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
    return hs::replay_row<McqLaneAccWays, true>(q, (uint32_t)(seed + qid), reinterpret_cast<uint64_t *>(out));
}

uint32_t hs_ways_row_bytes(void) { return (uint32_t)sizeof(mcq_result_ways); }
}
