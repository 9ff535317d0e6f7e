// hs_dealing.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the dealing's single-hole step (neuron_poker_amd/csrc/mcq_device.hpp: mcq_hole_pair) beside the generic
// scan and inserts it stands for (mcq_hole_put, mcq_hole_reg), and of the plain path's iteration walked lane by lane as
// the bulk kernel walks it, with a draw policy that hands McqCtrDraws' draws through and counts the cases the single-hole
// step can get wrong.
#include "../hostsim/hs_walk.hpp"

namespace {

// the register's second draw by the generic path: insert of the first at slot J - 1, scan, insert at slot J
template <int J>
void generic_step(uint32_t t0, uint32_t r, uint32_t *k, uint32_t *h) {
    uint32_t hh = MCQ_HOLE_SENTINEL, kk = r | 0x80u;
    mcq_hole_put<J - 1>(hh, t0 | 0x80u);
    mcq_hole_reg(mcq_splat_byte(r | 0x80u), hh, kk);
    mcq_hole_put<J>(hh, r | 0x80u);
    *k = kk;
    *h = hh;
}

// McqCtrDrawsT<UNIFORM> with counters.  hits[4 * site + what]: site 0..2 = opponent draws J = 1, 5, 9 (pairs 0, 2, 4), site 3 = table
// draw K = 1; what 0: r2 == r1, 1: r2 == r1 - 1, 2: the a == c branch (r1 = dd), 3: draws seen at the site
template <bool UNIFORM>
struct CountingDraws {
    static constexpr uint32_t kTableShort = McqCtrDrawsT<UNIFORM>::kTableShort;
    McqCtrDrawsT<UNIFORM> d;
    uint64_t *hits;
    uint32_t t0;
    void start(uint64_t seed, uint64_t qid, uint32_t stream) { d.start(seed, qid, stream); }
    template <int P>
    void pair(uint32_t L, uint32_t &r1, uint32_t &r2) {
        d.template pair<P>(L, r1, r2);
        if (P % 2 == 0 && P <= 4) {
            uint64_t *h = hits + 4 * (P / 2);
            h[0] += r2 == r1;
            h[1] += r2 + 1u == r1;
            h[2] += !UNIFORM && r1 == L - 1u + 128u;
            h[3] += 1;
        }
    }
    template <int K>
    uint32_t table(uint32_t n) {
        const uint32_t v = d.template table<K>(n);
        if (K == 0) t0 = v;
        if (K == 1) {
            hits[12] += v == t0;
            hits[13] += v + 1u == t0;
            hits[15] += 1;
        }
        return v;
    }
};

template <bool STRAIGHT, bool UNIFORM>
int run(const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row, uint64_t *hits) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    typedef CountingDraws<UNIFORM> Draws;
    const McqTables &t = hs::luts();
    const hs::BaseDeck bd(*q);
    Draws proto = {};
    proto.hits = hits;
    hs::walk_streams<Draws, McqLaneAcc>(bd.qc, q->runs, seed, qid, row, [&](Draws &dr, McqLaneAcc &acc, uint32_t cnt) {
        mcq_iterations<STRAIGHT>(bd.qc, dr, bd.card, t.tf, t.tops, t.sd, acc, cnt);
    }, proto);
    return MCQ_OK;
}
}  // namespace

// the second draw r into a register that holds the first, t0, alone: position count k and the register afterwards, by
// mcq_hole_pair (out[0], out[1]) and by the generic path at opponent draw J = 1, 5, 9 or, J = 0, at table draw K = 1
// (out[2], out[3])
extern "C" int hs_dealing_step(uint32_t j, uint32_t t0, uint32_t r, uint32_t *out) {
    uint32_t h = t0 | 0x80u, k = r | 0x80u; /* as mcq_draw_opp<J - 1> / mcq_draw_table<0> leave the register */
    mcq_hole_pair(r | 0x80u, h, k);
    out[0] = k;
    out[1] = h;
    switch (j) {
        case 0: case 1: generic_step<1>(t0, r, out + 2, out + 3); return 0;
        case 5: generic_step<5>(t0, r, out + 2, out + 3); return 0;
        case 9: generic_step<9>(t0, r, out + 2, out + 3); return 0;
        default: return -1;
    }
}
// row: runs, passes, win, tie, by_type[9]; straight != 0: the straight-line forms the bulk kernel runs, else the general
// form; uniform != 0: the opt-in uniform dealing law, else the reference's; hits[16] are ADDED to (see CountingDraws)
extern "C" int hs_dealing_run(const mcq_query *q, uint64_t seed, uint64_t qid, int straight, int uniform, uint64_t *row,
                              uint64_t *hits) {
    if (uniform) return straight ? run<true, true>(q, seed, qid, row, hits) : run<false, true>(q, seed, qid, row, hits);
    return straight ? run<true, false>(q, seed, qid, row, hits) : run<false, false>(q, seed, qid, row, hits);
}
