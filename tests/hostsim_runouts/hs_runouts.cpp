// hs_runouts.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the lane code of the per-runout exact enumeration (neuron_poker_amd/csrc/mcq_exact_runout.hpp) for the HOST
// compiler and walks the decomposition of mcq_exact_runout_kernel and mcq_exact_runout_cards_kernel on the CPU --
// completion by completion: a lane per completion without a random opponent, the 64 lanes of a wave over the candidate
// hands with one -- so that the GPU's rows can be pinned bit for bit and the lane code checked against independent walks
// in a container without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_runout.hpp"

// -> 0, -1 (bad law), the refusal MCQ_XX_* / MCQ_XR_* (1..7) or 8 = the range cannot be dealt.  cards: 52 x 22 words,
// pairs: 1326 x 22 words; both untouched by a refusal.
extern "C" int hs_runouts(const mcq_query *q, const mcq_query_ext *x, int law, uint64_t *cards_out, uint64_t *pairs_out) {
    const McqTables &t = hs::luts();
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return -1;
    const int why = mcq_exact_runout_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    memset(r_id, 0, sizeof r_id);
    mcq_exact_ext_r_ids(e, r_id);
    if (!mcq_exact_ext_dealable(e, r_id)) return 8;
    std::vector<uint8_t> cb_tab(MCQ_XX_MAX_RP);
    mcq_exact_ext_cb_table(e, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> pair_xy(MCQ_EXACT_PAIRS);
    for (uint32_t i = 0; i < MCQ_EXACT_PAIRS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    std::vector<unsigned long long> cards((size_t)MCQ_XR_CARD_ROWS * MCQ_XR_WORDS, 0ull), pairs((size_t)MCQ_XR_PAIR_ROWS * MCQ_XR_WORDS, 0ull);
    const uint32_t n_boards = mcq_exact_binom(e.b.L, e.b.k);
    for (uint32_t board = 0; board < n_boards; board++) {
        uint32_t slot, type, n_eq, win, tie, tot, tie_c = 0;
        if (e.b.n_opp == 0u) { /* mcq_exact_runout_kernel<0>: the lane that owns the completion */
            McqExactAcc a = {0, 0, 0};
            slot = mcq_exact_runout_lone(e, board, r_id, t.sel8, t.tf, t.tops, t.sd, a, type, n_eq);
            win = a.win; tie = a.tie; tot = a.tot;
        } else { /* mcq_exact_runout_kernel<1>: the wave that owns it */
            uint32_t pos[5];
            mcq_exact_unrank(board, e.b.L, e.b.k, pos);
            McqExactBoard bd;
            mcq_exact_board(e.b, pos, t.sel8, t.tf, t.tops, t.sd, bd);
            const uint32_t kb = mcq_exact_ext_known_best_eq(e, bd, t.tf, t.tops, t.sd, n_eq);
            McqCard rem_card[64];
            uint32_t rem_pos[64];
            for (uint32_t l = 0; l < e.m; l++) {
                rem_pos[l] = mcq_exact_rem_pos(pos, l);
                rem_card[l] = mcq_card(r_id[rem_pos[l]]);
            }
            McqExactAccWays acc = {0, 0, 0, 0}; /* (the wave sums: one accumulator over the 64 lanes) */
            for (uint32_t lane = 0; lane < 64; lane++)
                mcq_exact_ext_pass_a(e, bd, kb, lane, 64u, pair_xy.data(), rem_card, rem_pos, cb_tab.data(), t.tf, t.tops, t.sd,
                                     (uint32_t *)nullptr, (uint32_t *)nullptr, acc);
            win = acc.win; tie = acc.tie; tot = acc.tot; tie_c = acc.tie_c;
            type = mcq_key_type(bd.hero_key);
            slot = mcq_exact_runout_slot(e, r_id, pos);
        }
        if (tot == 0u) continue;
        if (slot >= MCQ_XR_ROWS) return 9;
        unsigned long long *row = mcq_exact_runout_row(cards.data(), pairs.data(), slot);
        for (uint32_t w = 0; w < MCQ_XR_WORDS; w++) {
            if (row[w] != 0ull) return 10; /* a slot with two owners */
            row[w] = mcq_exact_runout_word(w, win, tie, tot, tie_c, type, n_eq);
        }
    }
    if (e.b.k == 2u) /* mcq_exact_runout_cards_kernel: thread (card, word) */
        for (uint32_t i = 0; i < MCQ_XR_CARD_ROWS * MCQ_XR_WORDS; i++)
            cards[i] = mcq_exact_runout_card_word(pairs.data(), i / MCQ_XR_WORDS, i % MCQ_XR_WORDS);
    memcpy(cards_out, cards.data(), cards.size() * 8u);
    memcpy(pairs_out, pairs.data(), pairs.size() * 8u);
    return 0;
}
