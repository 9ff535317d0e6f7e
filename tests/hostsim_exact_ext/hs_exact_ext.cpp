// hs_exact_ext.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the lane code of the extended exact enumeration (neuron_poker_amd/csrc/mcq_exact_ext.hpp) for the HOST
// compiler and walks mcq_exact_ext_kernel's decomposition sequentially -- completion by completion, the lanes one after
// the other -- and finishes the sums as the library's host side does, so that the GPU's output can be pinned bit for bit
// and the lane code checked against an independent walk of the reference in a container that has no GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_ext.hpp"

// -> 0, or the refusal: MCQ_XX_* (1..4), 5 = the range cannot be dealt.  prob: 11 doubles, weights: 13 words.
extern "C" int hs_exact_ext(const mcq_query *q, const mcq_query_ext *x, int law, double *prob, uint64_t *weights) {
    const McqTables &t = hs::luts();
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    const int why = mcq_exact_ext_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e, r_id);
    if (!mcq_exact_ext_dealable(e, r_id)) return 5;
    std::vector<uint8_t> cb_tab(MCQ_XX_MAX_RP);
    mcq_exact_ext_cb_table(e, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> pair_xy(MCQ_EXACT_PAIRS);
    std::vector<uint32_t> keys(MCQ_EXACT_PAIRS), rec(MCQ_EXACT_PAIRS);
    for (uint32_t i = 0; i < MCQ_EXACT_PAIRS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    std::vector<unsigned long long> h1((size_t)e.n_rp * MCQ_XX_SUMS, 0ull);
    mcq_result w;
    memset(&w, 0, sizeof w);
    const uint32_t n_boards = mcq_exact_binom(e.b.L, e.b.k);
    for (uint32_t board = 0; board < n_boards; board++) {
        McqExactAcc acc = {0, 0, 0};
        uint32_t type;
        if (e.b.n_opp == 0u) {
            type = mcq_exact_ext_lone(e, board, t.sel8, t.tf, t.tops, t.sd, acc);
        } else {
            uint32_t pos[5];
            mcq_exact_unrank(board, e.b.L, e.b.k, pos);
            McqExactBoard bd;
            mcq_exact_board(e.b, pos, t.sel8, t.tf, t.tops, t.sd, bd);
            type = mcq_key_type(bd.hero_key);
            const uint32_t kb = mcq_exact_ext_known_best(e, bd, t.tf, t.tops, t.sd);
            McqCard rem_card[64];
            uint32_t rem_pos[64];
            for (uint32_t l = 0; l < e.m; l++) {
                rem_pos[l] = mcq_exact_rem_pos(pos, l);
                rem_card[l] = mcq_card(r_id[rem_pos[l]]);
            }
            const bool two = e.b.n_opp == 2u;
            for (uint32_t lane = 0; lane < 64; lane++)
                mcq_exact_ext_pass_a(e, bd, kb, lane, 64u, pair_xy.data(), rem_card, rem_pos, cb_tab.data(), t.tf, t.tops, t.sd,
                                     two ? keys.data() : nullptr, rec.data(), acc);
            if (two) {
                for (uint32_t h = 0; h < e.n_rp; h++) {
                    uint32_t qa, qb;
                    mcq_exact_pair_xy(h, qa, qb);
                    const uint32_t mi = mcq_exact_ext_m_index(e, pos, qa, qb);
                    if (mi >= e.n_pairs) continue;
                    McqExactAcc a = {0, 0, 0};
                    mcq_exact_ext_pass_b(e, bd, qa, qb, mi, keys.data(), rec.data(), a);
                    McqExactExtSums s = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
                    mcq_exact_ext_add(s, a, type);
                    unsigned long long *dst = &h1[(size_t)h * MCQ_XX_SUMS];
                    dst[0] += s.win;
                    dst[1] += s.tie;
                    dst[2] += s.tot;
                    for (int k = 0; k < 9; k++) dst[3 + k] += s.type[k];
                }
                continue;
            }
        }
        w.runs += acc.tot;
        w.win += acc.win;
        w.tie += acc.tie;
        w.by_type[type] += acc.win + acc.tie;
    }
    mcq_exact_prob p;
    mcq_exact_ext_finish(e, r_id, h1.data(), w, p);
    memcpy(prob, &p, sizeof p);
    memcpy(weights, &w, sizeof w);
    return 0;
}

// R-positions' card ids, first-hand weights w1 and the per-first-hand sums of a two-opponent query (n_rp x 12); -> n_rp
extern "C" int hs_exact_ext_r(const mcq_query *q, const mcq_query_ext *x, int law, uint8_t *r_id_out) {
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (mcq_exact_ext_query(mcq_query_words(*q), er, law, e)) return -1;
    mcq_exact_ext_r_ids(e, r_id_out);
    return (int)e.b.L;
}
