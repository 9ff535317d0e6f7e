// mcq_exact_runout.hpp -- exact equity PER RUNOUT (mcq_exact_batch_ext_runouts): the split-pot enumeration of
// mcq_exact_ext.hpp, kinds 0 and 1, with the sums of every table completion kept apart instead of folded into one row;
// lane code shared by mcq_exact_runout_kernel / mcq_exact_runout_cards_kernel (mcq_kernels.hip) and the host build of the
// tests (tests/hostsim_runouts).  mcq_exact.hpp and mcq_exact_ext.hpp are reused unchanged: a completion's row words are
// mcq_exact_ext_row_word's, the same function that gives the folded rows of mcq_exact_ext_kernel.
//
// Flop (k = 2 cards to come) and turn (k = 1) only.  Per record the device keeps MCQ_XR_ROWS zeroed rows of 22 words
// (mcq_result_ways): 52 card rows and MCQ_HAND_ROWS pair rows (slots 0..51 and 52..1377).  A completion has exactly ONE
// owner -- a lane (kind 0: no random opponent) or a wave (kind 1: one random opponent, lanes over the candidate hands) --
// which stores the completion's row once into the slot named by the card ids of the completion:
//   k = 1  card row r_id[pos[0]];
//   k = 2  pair row MCQ_HAND_INDEX(r_id[pos[0]], r_id[pos[1]]) (positions ascend, and so do R's card ids).
// A completion without weight (the reference law: its highest card is the highest card left for every opponent hand)
// stores nothing: the row stays zero, as do the rows of the cards and pairs outside R.  For k = 2 the card rows are the
// sums of the pair rows that hold the card (mcq_exact_runout_card_word), made by a second kernel.
#ifndef MCQ_EXACT_RUNOUT_HPP
#define MCQ_EXACT_RUNOUT_HPP

#include "mcq_exact_ext.hpp"

#define MCQ_XR_CARD_ROWS 52u
#define MCQ_XR_PAIR_ROWS 1326u /* MCQ_HAND_ROWS */
#define MCQ_XR_ROWS (MCQ_XR_CARD_ROWS + MCQ_XR_PAIR_ROWS)
#define MCQ_XR_WORDS 22u       /* 64-bit words of an mcq_result_ways row */

/* why a record has no per-runout form (after MCQ_XX_*) */
#define MCQ_XR_TWO_OPP 5
#define MCQ_XR_PREFLOP 6
#define MCQ_XR_RIVER 7

MCQ_HD int mcq_exact_runout_query(const McqQueryWords &q, const McqExtRec &er, int law, McqExactExtQuery &e) {
    const int why = mcq_exact_ext_query(q, er, law, e);
    if (why != MCQ_XX_OK) return why;
    if (e.b.n_opp > 1u) return MCQ_XR_TWO_OPP;
    if (e.b.k == 5u) return MCQ_XR_PREFLOP;
    if (e.b.k == 0u) return MCQ_XR_RIVER;
    return MCQ_XX_OK;
}

// the row (of the record's MCQ_XR_ROWS) that owns the completion at ascending R-positions pos[0..k)
MCQ_HD uint32_t mcq_exact_runout_slot(const McqExactExtQuery &e, const uint8_t *r_id, const uint32_t pos[5]) {
    const uint32_t a = r_id[pos[0] & 63u];
    if (e.b.k == 1u) return a;
    const uint32_t b = r_id[pos[1] & 63u]; /* (k = 1: entry 1 is 255, never read as a position) */
    return MCQ_XR_CARD_ROWS + MCQ_HAND_INDEX(a, b);
}

// that row's words: a record's card rows and pair rows lie apart
MCQ_HD unsigned long long *mcq_exact_runout_row(unsigned long long *cards, unsigned long long *pairs, uint32_t slot) {
    return slot < MCQ_XR_CARD_ROWS ? cards + (size_t)slot * MCQ_XR_WORDS : pairs + (size_t)(slot - MCQ_XR_CARD_ROWS) * MCQ_XR_WORDS;
}

// a completion's row words, by the name the host simulator of the tests calls
MCQ_HD unsigned long long mcq_exact_runout_word(uint32_t word, uint32_t win, uint32_t tie, uint32_t tot, uint32_t tie_c,
                                                uint32_t type, uint32_t n_eq) {
    return mcq_exact_ext_row_word(word, win, tie, tot, tie_c, type, n_eq);
}

// Kind 0, one lane: completion `idx` alone -> its slot; a (OUT: set, not added to), type and n_eq are its sums (weight 0 or 1)
MCQ_HD uint32_t mcq_exact_runout_lone(const McqExactExtQuery &e, uint32_t idx, const uint8_t *r_id, const uint32_t *sel8,
                                      const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, McqExactAcc &a,
                                      uint32_t &type, uint32_t &n_eq) {
    uint32_t pos[5];
    McqExactBoard bd;
    McqExactKnown kn;
    const uint32_t w = mcq_exact_ext_lone_known(e, idx, sel8, tf, tops, sd, pos, bd, kn);
    a = mcq_exact_ext_lone_acc(bd, kn, w);
    type = mcq_key_type(bd.hero_key);
    n_eq = kn.n_eq;
    return mcq_exact_runout_slot(e, r_id, pos);
}

// k = 2: word `word` of card row c = the pair rows that hold c, added in ascending order of the other card (rows of pairs
// that cannot come are zero); pairs -> the record's MCQ_XR_PAIR_ROWS x MCQ_XR_WORDS words
MCQ_HD unsigned long long mcq_exact_runout_card_word(const unsigned long long *pairs, uint32_t c, uint32_t word) {
    unsigned long long s = 0;
    for (uint32_t o = 0; o < 52u; o++) {
        if (o == c) continue;
        const uint32_t a = o < c ? o : c, b = o < c ? c : o;
        s += pairs[(size_t)MCQ_HAND_INDEX(a, b) * MCQ_XR_WORDS + word];
    }
    return s;
}

#endif /* MCQ_EXACT_RUNOUT_HPP */
