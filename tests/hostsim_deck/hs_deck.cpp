// hs_deck.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of two pieces of the plain path's lane code (neuron_poker_amd/csrc/mcq_device.hpp): the position arithmetic
// of the dealing (mcq_draw_opp, mcq_draw_table) and the two deck accessors of the
// iteration (McqDeckAoS, McqDeckSplit), run side by side on the same streams.
#include "../hostsim/hs_walk.hpp"

namespace {
constexpr uint32_t kY = 1024u + 1u; /* as the kernels lay it out: no multiple of 64, beyond 255 entries */
typedef McqDeckSplit<kY> Split;

template <int K>
uint32_t draw(uint32_t r, const uint32_t (&H)[5], uint32_t &hb) { return mcq_draw_table<K, 0>(r | 0x80u, H, hb) & 0x7Fu; }

template <class Draws, class Acc, bool STRAIGHT, class Deck>
void run(const McqQueryCtx &qc, const McqTables &t, const Deck &deck, uint64_t seed, uint64_t qid, uint32_t runs, std::vector<Acc> &out) {
    const McqSumTabs tabs = mcq_sum_tabs_of(t.tf);
    hs::each_stream<Draws, Acc>(runs, seed, qid, [&](Draws &dr, Acc &acc, uint32_t cnt) { /* the lanes' own sums, not a row */
        if (STRAIGHT) mcq_iterations_sum<true>(qc, dr, deck, tabs, acc, cnt);
        else for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, -1, -1, Acc>(qc, dr, deck, tabs, acc);
        out.push_back(acc);
    });
}
template <class Draws, class Acc, bool STRAIGHT>
int64_t both(const mcq_query *q, uint64_t seed, uint64_t qid) {
    if (!mcq_query_valid(mcq_query_words(*q))) return -1;
    const McqTables &t = hs::luts();
    const hs::BaseDeck bd(*q);
    const McqQueryCtx &qc = bd.qc;
    std::vector<McqPair> split(128 + 64 + kY + 64);
    for (uint32_t l = 0; l < 64; l++) Split::put(split.data() + 128, l, bd.card[128 + l]);
    const McqDeckAoS da = bd.aos();
    const Split ds = {split.data()};
    std::vector<Acc> a, b;
    run<Draws, Acc, STRAIGHT>(qc, t, da, seed, qid, q->runs, a);
    run<Draws, Acc, STRAIGHT>(qc, t, ds, seed, qid, q->runs, b);
    int64_t bad = 0, any = 0;
    for (size_t i = 0; i < a.size(); i++) {
        bad += memcmp(&a[i], &b[i], sizeof(Acc)) != 0;
        any += a[i].types != 0;
    }
    return bad ? -2 - bad : any; /* >= 0: the streams that counted a win, all equal */
}
// one iteration's deal: the opponents' draws r[0 .. 2 n_opp), then the table's -> base positions (as the iteration forms them)
template <int P>
void deal_opps(uint32_t n_opp, const uint8_t *r, uint8_t *pos, uint32_t (&H)[5]) {
    if constexpr (P < (int)MCQ_MAX_OPP) {
        if ((uint32_t)P < n_opp) {
            pos[2 * P] = (uint8_t)(mcq_draw_opp<2 * P>(r[2 * P] | 0x80u, H) & 0x7Fu);
            pos[2 * P + 1] = (uint8_t)(mcq_draw_opp<2 * P + 1>(r[2 * P + 1] | 0x80u, H) & 0x7Fu);
            deal_opps<P + 1>(n_opp, r, pos, H);
        }
    }
}
template <int NREGS>
void deal_table(uint32_t n_deal, const uint8_t *r, uint8_t *pos, const uint32_t (&H)[5]) {
    uint32_t rt = MCQ_HOLE_SENTINEL; /* the table's own holes */
    if (n_deal > 0) pos[0] = (uint8_t)(mcq_draw_table<0, NREGS>(r[0] | 0x80u, H, rt) & 0x7Fu);
    if (n_deal > 1) pos[1] = (uint8_t)(mcq_draw_table<1, NREGS>(r[1] | 0x80u, H, rt) & 0x7Fu);
    if (n_deal > 2) pos[2] = (uint8_t)(mcq_draw_table<2, NREGS>(r[2] | 0x80u, H, rt) & 0x7Fu);
    if (n_deal > 3) pos[3] = (uint8_t)(mcq_draw_table<3, NREGS>(r[3] | 0x80u, H, rt) & 0x7Fu);
    if (n_deal > 4) pos[4] = (uint8_t)(mcq_draw_table<4, NREGS>(r[4] | 0x80u, H, rt) & 0x7Fu);
}
}  // namespace

extern "C" {
// `count` iterations of n_opp opponents and n_deal table cards: rows of 2 n_opp + n_deal draws -> rows of base positions
void hs_deal_many(uint32_t n_opp, uint32_t n_deal, const uint8_t *r, uint64_t count, uint8_t *pos) {
    const uint32_t D = 2u * n_opp + n_deal;
    for (uint64_t i = 0; i < count; i++) {
        uint32_t H[5] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
        deal_opps<0>(n_opp, r + i * D, pos + i * D, H);
        const uint8_t *rt = r + i * D + 2u * n_opp;
        uint8_t *pt = pos + i * D + 2u * n_opp;
        switch ((2u * n_opp + 3u) / 4u) { /* registers holding the opponents' holes, as mcq_iteration_sum picks */
            case 0: deal_table<0>(n_deal, rt, pt, H); break;
            case 1: deal_table<1>(n_deal, rt, pt, H); break;
            case 2: deal_table<2>(n_deal, rt, pt, H); break;
            case 3: deal_table<3>(n_deal, rt, pt, H); break;
            case 4: deal_table<4>(n_deal, rt, pt, H); break;
            default: deal_table<5>(n_deal, rt, pt, H); break;
        }
    }
}
// positions (in the list as the opponents left it) of the n table draws r[0..n), as mcq_draw_table computes them
void hs_unpop(const uint8_t *r, uint32_t n, uint8_t *pos) {
    const uint32_t H[5] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
    uint32_t R = MCQ_HOLE_SENTINEL; /* the table's own holes */
    if (n > 0) pos[0] = (uint8_t)draw<0>(r[0], H, R);
    if (n > 1) pos[1] = (uint8_t)draw<1>(r[1], H, R);
    if (n > 2) pos[2] = (uint8_t)draw<2>(r[2], H, R);
    if (n > 3) pos[3] = (uint8_t)draw<3>(r[3], H, R);
    if (n > 4) pos[4] = (uint8_t)draw<4>(r[4], H, R);
}
// ... for `count` sequences at once (rows of n)
void hs_unpop_many(const uint8_t *r, uint32_t n, uint64_t count, uint8_t *pos) {
    for (uint64_t i = 0; i < count; i++) hs_unpop(r + i * n, n, pos + i * n);
}
// the iterations of a query through both accessors; law: 0 reference, 1 uniform; ways: split-pot accumulator;
// general: the general form.  >= 0: lane accumulators equal (the number of them that hold a win), < 0: not
int64_t hs_deck_both(const mcq_query *q, uint64_t seed, uint64_t qid, int law, int ways, int general) {
#define PICK(D) (ways ? (general ? both<D, McqLaneAccWays, false>(q, seed, qid) : both<D, McqLaneAccWays, true>(q, seed, qid)) \
                      : (general ? both<D, McqLaneAcc, false>(q, seed, qid) : both<D, McqLaneAcc, true>(q, seed, qid)))
    return law ? PICK(McqCtrDrawsUniform) : PICK(McqCtrDraws);
#undef PICK
}
}
