// hs_bysuit.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the opponents' cards read by flush suit (neuron_poker_amd/csrc/mcq_device.hpp: mcq_hole_entry, hole_by_suit
// of the deck accessors, McqDeckBySuit and its hole table, the BYSUIT forms of mcq_iteration_sum).
//   * hs_bysuit_entries: the hole table of a query's base deck, filled as the bulk kernel fills it (put_holes) in either
//     layout and read back through hole_by_suit, beside what McqSumHole::set and the v_perm of mcq_sum_first extract from
//     the same McqCard -- every position, every suit -- and beside the accessors that derive the entry from the card.
//   * hs_bysuit_run: one query through mcq_iteration_sum<Draws, nopp, ndeal, Acc, Deck, rule, BYSUIT> as the bulk kernel
//     walks it, with the accessor NAMED by the caller: the cards read where they are dealt (BYSUIT false, the array of
//     cards), or by suit from the array of cards, from a position-major or from a suit-major hole table.
#include "../hostsim/hs_walk.hpp"

namespace {
// HS_BYSUIT_LEAN (hs_main.cpp, the stand-alone program under the sanitizers): a few forms -- heads-up with one card to
// come, 6-max with five to come and with a run-time count, ten players; split-pot rows under the reference law only -- so
// that the instrumented build does not take minutes.
#ifdef HS_BYSUIT_LEAN
struct Forms {
    static constexpr bool has(bool uniform, bool ways, int nopp, int ndeal) {
        return !(uniform && ways) && ((nopp == 1 && ndeal == 1) || (nopp == 5 && (ndeal == 5 || ndeal == -1)) || (nopp == 9 && ndeal == -1));
    }
};
#else
typedef hs::StraightForms Forms;
#endif
constexpr uint32_t kY = 1024u + 1u; /* as the kernels lay the base decks out */
typedef McqDeckBySuit<kY, 5u, 8u> DeckPos;                        /* position-major */
typedef McqDeckBySuit<kY, 3u, 8u * MCQ_HOLE_POSITIONS> DeckSuit;  /* suit-major */
typedef McqDeckSplit<kY> DeckSplit;


// a query's base deck behind every accessor: the array of cards, the two arrays of halves, and a hole table per layout.
// A table's 1600 bytes END its heap block (a read or write behind position 49 is the sanitizer's); in front of it lie the
// 128 positions of the bias that `at` carries, so that the biased pointer is the block's own
struct Decks : hs::BaseDeck {
    std::vector<McqPair> split;
    std::vector<char> hpos, hsuit;
    explicit Decks(const mcq_query &q)
        : hs::BaseDeck(q), split(128 + 64 + kY + 64), hpos((128u << 5) + MCQ_HOLE_WAVE_BYTES), hsuit((128u << 3) + MCQ_HOLE_WAVE_BYTES) {
        for (uint32_t l = 0; l < 63u; l++) { /* as mcq_eval_kernel fills them */
            DeckPos::put(split.data() + 128, l, card[128 + l]);
            if (l < MCQ_HOLE_POSITIONS) {
                DeckPos::put_holes(hpos.data() + (128u << 5), l, card[128 + l]);
                DeckSuit::put_holes(hsuit.data() + (128u << 3), l, card[128 + l]);
            }
        }
    }
    DeckSplit deck_split() const { return DeckSplit{split.data()}; }
    DeckPos deck_pos() const { return DeckPos{{split.data()}, hpos.data()}; }
    DeckSuit deck_suit() const { return DeckSuit{{split.data()}, hsuit.data()}; }
};

template <class F, bool BYSUIT, class Deck>
int run(const Decks &dk, const Deck &deck, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    const McqSumTabs tabs = mcq_sum_tabs_of(hs::luts().tf);
    return F::walk(dk.qc, q->runs, seed, qid, row, [&](typename F::Draws &dr, typename F::Acc &acc) {
        mcq_iteration_sum<typename F::Draws, F::kNopp, F::kNdeal, typename F::Acc, Deck, MCQ_DEAL_RULE, BYSUIT>(dk.qc, dr, deck, tabs, acc);
    });
}
}  // namespace

extern "C" {

int hs_bysuit_default(void) { return MCQ_HOLE_BY_SUIT; }
uint32_t hs_bysuit_rank_weight2(uint32_t rank) { return 2u * mcq_rank_weight(rank); }
uint32_t hs_bysuit_wave_bytes(void) { return MCQ_HOLE_WAVE_BYTES; }

// The base deck of q, positions 0 .. 49 x suits 0 .. 3, two words an entry.  out[0]: what today's reading extracts from the
// position's McqCard (McqSumHole::set with no second card, then the v_perm by the selector McqFlushSel forms for a table
// with three cards of that suit); out[1]: mcq_hole_entry through the array of cards; out[2]: through the two arrays of
// halves; out[3] / out[4]: the position-major / suit-major hole table, filled by put_holes and read by hole_by_suit.
// Every out[k] is [50][4][2].  Returns the deck's length, or a negative number.
int hs_bysuit_entries(const mcq_query *q, uint32_t *out) {
    if (!mcq_query_valid(mcq_query_words(*q))) return -1;
    const Decks dk(*q);
    const McqDeckAoS da = dk.aos();
    const DeckSplit ds = dk.deck_split();
    const DeckPos dp = dk.deck_pos();
    const DeckSuit du = dk.deck_suit();
    const McqCard none = {0u, 0u, 0u, 0u};
    const uint32_t n = MCQ_HOLE_POSITIONS * 4u * 2u;
    for (uint32_t p = 0; p < MCQ_HOLE_POSITIONS; p++)
        for (uint32_t s = 0; s < 4u; s++) {
            McqSumBoard b;
            b.clear();
            b.cnt = 3u << (4u * s); /* three table cards of suit s */
            McqFlushSel fs;
            if (fs.from_board_suit(b) != s) return -2;
            McqFlushSel fs2;
            fs2.from_board(b);
            if (fs2.psel != fs.psel || fs2.bfl4 != fs.bfl4) return -3;
            McqSumHole h;
            h.set(da.hole_card(128u + p), none);
            uint32_t *o = out + (p * 4u + s) * 2u;
            o[0] = h.ksum;
            o[1] = mcq_perm(h.his, h.los, fs.psel);
            const McqPair e1 = da.hole_by_suit(128u + p, da.suit_key(s)), e2 = ds.hole_by_suit(128u + p, ds.suit_key(s)),
                          e3 = dp.hole_by_suit(128u + p, dp.suit_key(s)), e4 = du.hole_by_suit(128u + p, du.suit_key(s));
            o[n] = e1.a, o[n + 1] = e1.b;
            o[2 * n] = e2.a, o[2 * n + 1] = e2.b;
            o[3 * n] = e3.a, o[3 * n + 1] = e3.b;
            o[4 * n] = e4.a, o[4 * n + 1] = e4.b;
        }
    return (int)dk.qc.L0;
}

// One query through mcq_iteration_sum<Draws, nopp, ndeal, Acc, Deck, the product's rule, BYSUIT>, nopp >= 1; ndeal -1 =
// counted at run time.  accessor: 0 the cards read where they are dealt (the array of cards); by suit: 1 from the array of
// cards, 2 from a position-major hole table, 3 from a suit-major one.  uniform != 0: the uniform dealing law.
// ways != 0: row = 22 words; else 13 words.
int hs_bysuit_run(const mcq_query *q, uint64_t seed, uint64_t qid, int nopp, int ndeal, int uniform, int ways, int accessor,
                  uint64_t *row) {
    if (!mcq_query_valid(mcq_query_words(*q))) return MCQ_EINVAL;
    return hs::for_form<Forms>(uniform, ways, nopp, ndeal, [&](auto form) -> int {
        typedef decltype(form) F;
        const Decks dk(*q);
        switch (accessor) {
            case 0: return run<F, false>(dk, dk.aos(), q, seed, qid, row);
            case 1: return run<F, true>(dk, dk.aos(), q, seed, qid, row);
            case 2: return run<F, true>(dk, dk.deck_pos(), q, seed, qid, row);
            case 3: return run<F, true>(dk, dk.deck_suit(), q, seed, qid, row);
            default: return MCQ_EINVAL;
        }
    });
}
}
