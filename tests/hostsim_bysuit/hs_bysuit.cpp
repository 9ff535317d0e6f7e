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
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace {
// HS_BYSUIT_LEAN (hs_main.cpp, the stand-alone program under the sanitizers): a few forms -- heads-up with one card to
// come, 6-max with five to come and with a run-time count, ten players -- so that the instrumented build does not take minutes.
#ifdef HS_BYSUIT_LEAN
constexpr bool kLean = true;
#else
constexpr bool kLean = false;
#endif
McqTables g_tab;
bool g_init = false;
const McqTables &luts() {
    if (!g_init) { mcq_fill_tables(&g_tab); g_init = true; }
    return g_tab;
}
constexpr uint32_t kY = 1024u + 1u; /* as the kernels lay the base decks out */
typedef McqDeckBySuit<kY, 5u, 8u> DeckPos;                        /* position-major */
typedef McqDeckBySuit<kY, 3u, 8u * MCQ_HOLE_POSITIONS> DeckSuit;  /* suit-major */
typedef McqDeckSplit<kY> DeckSplit;


// a query's base deck behind every accessor: the array of cards, the two arrays of halves, and a hole table per layout.
// A table's 1600 bytes END its heap block (a read or write behind position 49 is the sanitizer's); in front of it lie the
// 128 positions of the bias that `at` carries, so that the biased pointer is the block's own
struct Decks {
    std::vector<McqCard> aos;
    std::vector<McqPair> split;
    std::vector<char> hpos, hsuit;
    McqQueryCtx qc;
    explicit Decks(const mcq_query &q) : aos(192), split(128 + 64 + kY + 64), hpos((128u << 5) + MCQ_HOLE_WAVE_BYTES), hsuit((128u << 3) + MCQ_HOLE_WAVE_BYTES) {
        const McqTables &t = luts();
        mcq_query_ctx(mcq_query_words(q), qc);
        for (uint32_t l = 0; l < 64; l++) {
            aos[128 + l] = mcq_base_entry(qc, l, t.sel8);
            if (l < 63u) { /* as mcq_eval_kernel fills them */
                DeckPos::put(split.data() + 128, l, aos[128 + l]);
                if (l < MCQ_HOLE_POSITIONS) {
                    DeckPos::put_holes(hpos.data() + (128u << 5), l, aos[128 + l]);
                    DeckSuit::put_holes(hsuit.data() + (128u << 3), l, aos[128 + l]);
                }
            }
        }
    }
    McqDeckAoS deck_aos() const { return McqDeckAoS{aos.data()}; }
    DeckSplit deck_split() const { return DeckSplit{split.data()}; }
    DeckPos deck_pos() const { return DeckPos{{split.data()}, hpos.data()}; }
    DeckSuit deck_suit() const { return DeckSuit{{split.data()}, hsuit.data()}; }
};

template <class Draws, class Acc, int NOPP, int NDEAL, bool BYSUIT, class Deck>
int run(const Decks &dk, const Deck &deck, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    const McqTables &t = luts();
    const McqQueryCtx &qc = dk.qc;
    if (qc.n_opp != (uint32_t)NOPP || (NDEAL >= 0 && qc.n_deal != (uint32_t)NDEAL)) return MCQ_EINVAL;
    const McqSumTabs tabs = mcq_sum_tabs_of(t.tf);
    memset(row, 0, (Acc::kWays ? 22 : 13) * sizeof(uint64_t));
    row[0] = q->runs;
    const uint32_t n_streams = (q->runs + MCQ_STREAM_ITERS - 1) / MCQ_STREAM_ITERS;
    for (uint32_t s = 0; s < n_streams; s++) {
        Draws dr;
        dr.start(seed, qid, s);
        Acc acc = {};
        const uint64_t left = (uint64_t)q->runs - (uint64_t)s * MCQ_STREAM_ITERS;
        const uint32_t cnt = left < MCQ_STREAM_ITERS ? (uint32_t)left : MCQ_STREAM_ITERS;
        for (uint32_t j = 0; j < cnt; j++)
            mcq_iteration_sum<Draws, NOPP, NDEAL, Acc, Deck, MCQ_DEAL_RULE, BYSUIT>(qc, dr, deck, tabs, acc);
        row[1] += (uint64_t)cnt * qc.n_opp; /* passes: one attempt per opponent, never re-drawn */
        mcq_tally_fold(acc, row);
    }
    return MCQ_OK;
}
template <class Draws, class Acc, int NOPP, int NDEAL>
int by_accessor(int accessor, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    const Decks dk(*q);
    switch (accessor) {
        case 0: return run<Draws, Acc, NOPP, NDEAL, false>(dk, dk.deck_aos(), q, seed, qid, row);
        case 1: return run<Draws, Acc, NOPP, NDEAL, true>(dk, dk.deck_aos(), q, seed, qid, row);
        case 2: return run<Draws, Acc, NOPP, NDEAL, true>(dk, dk.deck_pos(), q, seed, qid, row);
        case 3: return run<Draws, Acc, NOPP, NDEAL, true>(dk, dk.deck_suit(), q, seed, qid, row);
        default: return MCQ_EINVAL;
    }
}
template <class Draws, class Acc, int NOPP>
int by_deal(int ndeal, int accessor, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if constexpr (kLean) {
        if constexpr (NOPP == 1) { if (ndeal == 1) return by_accessor<Draws, Acc, 1, 1>(accessor, q, seed, qid, row); }
        if constexpr (NOPP == 5) { if (ndeal == 5) return by_accessor<Draws, Acc, 5, 5>(accessor, q, seed, qid, row); }
        if constexpr (NOPP == 5 || NOPP == 9) { if (ndeal == -1) return by_accessor<Draws, Acc, NOPP, -1>(accessor, q, seed, qid, row); }
        return MCQ_EINVAL;
    }
    if (ndeal == -1) return by_accessor<Draws, Acc, NOPP, -1>(accessor, q, seed, qid, row);
    if constexpr (NOPP <= 7) { /* the instantiations mcq_iterations_sum has */
        if (ndeal == 5) return by_accessor<Draws, Acc, NOPP, 5>(accessor, q, seed, qid, row);
        if (ndeal == 2) return by_accessor<Draws, Acc, NOPP, 2>(accessor, q, seed, qid, row);
        if (ndeal == 1) return by_accessor<Draws, Acc, NOPP, 1>(accessor, q, seed, qid, row);
    }
    return MCQ_EINVAL;
}
template <class Draws, class Acc>
int by_opp(int nopp, int ndeal, int accessor, const mcq_query *q, uint64_t seed, uint64_t qid, uint64_t *row) {
    if constexpr (kLean) {
        if (nopp == 1) return by_deal<Draws, Acc, 1>(ndeal, accessor, q, seed, qid, row);
        if (nopp == 5) return by_deal<Draws, Acc, 5>(ndeal, accessor, q, seed, qid, row);
        if (nopp == 9) return by_deal<Draws, Acc, 9>(ndeal, accessor, q, seed, qid, row);
        return MCQ_EINVAL;
    } else switch (nopp) {
        case 1: return by_deal<Draws, Acc, 1>(ndeal, accessor, q, seed, qid, row);
        case 2: return by_deal<Draws, Acc, 2>(ndeal, accessor, q, seed, qid, row);
        case 3: return by_deal<Draws, Acc, 3>(ndeal, accessor, q, seed, qid, row);
        case 4: return by_deal<Draws, Acc, 4>(ndeal, accessor, q, seed, qid, row);
        case 5: return by_deal<Draws, Acc, 5>(ndeal, accessor, q, seed, qid, row);
        case 6: return by_deal<Draws, Acc, 6>(ndeal, accessor, q, seed, qid, row);
        case 7: return by_deal<Draws, Acc, 7>(ndeal, accessor, q, seed, qid, row);
        case 8: return by_deal<Draws, Acc, 8>(ndeal, accessor, q, seed, qid, row);
        case 9: return by_deal<Draws, Acc, 9>(ndeal, accessor, q, seed, qid, row);
        default: return MCQ_EINVAL;
    }
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
    const McqDeckAoS da = dk.deck_aos();
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
    if constexpr (kLean) {
        if (uniform && ways) return MCQ_EINVAL;
        if (uniform) return by_opp<McqCtrDrawsUniform, McqLaneAcc>(nopp, ndeal, accessor, q, seed, qid, row);
    } else if (uniform)
        return ways ? by_opp<McqCtrDrawsUniform, McqLaneAccWays>(nopp, ndeal, accessor, q, seed, qid, row)
                    : by_opp<McqCtrDrawsUniform, McqLaneAcc>(nopp, ndeal, accessor, q, seed, qid, row);
    return ways ? by_opp<McqCtrDraws, McqLaneAccWays>(nopp, ndeal, accessor, q, seed, qid, row)
                : by_opp<McqCtrDraws, McqLaneAcc>(nopp, ndeal, accessor, q, seed, qid, row);
}
}
