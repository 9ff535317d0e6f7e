// mcq_exact_hero_pre.hpp -- exact enumeration with the HERO given as a range BEFORE THE FLOP: every hero hand against one
// random opponent (ranged or not) from ONE enumeration of the C(|D|, 5) table completions; lane code shared by
// mcq_exact_hero_pre_kernel and mcq_exact_hero_pre_w_kernel (mcq_kernels.hip) and the host builds of the tests
// (tests/hostsim_hero_preflop, tests/hostsim_hero_preflop_weighted).
//
// The mathematics is mcq_exact_hero.hpp's -- its opening comment is the specification: the opponent's weight is
// mcq_exact_ext_w2 with the hero's hand as the hand that left the deck, under MCQ_LAW_REFERENCE a completion counts iff
// above(h) + above(o) < u, and a hero hand's sums are win, tie, tot and by_type[9].  mcq_exact.hpp, mcq_exact_ext.hpp and
// mcq_exact_hero.hpp are included and reused unchanged.  The code is generic in k = 0..5 new table cards (the C entry takes
// k = 5 only), so that the tests can pin it against mcq_exact_hero.hpp on the flop, turn and river.
//
// What differs.  D = 52 cards minus table and ghost, |D| <= 52: up to C(52, 2) = 1326 hero hands, up to C(52, 5) =
// 2 598 960 completions, each leaving C(|D| - k, 2) <= 1081 hands.  Nothing is indexed by the per-completion m-index:
// every hand is a D-PAIR (D-positions pa < pb, index pb (pb - 1) / 2 + pa), fixed across the completions, and a
// completion only marks the pairs that touch one of its table cards as dead (key 0 -- every hand's key is > 0 -- and
// record 0, whose range bits give weight 0 under both laws).  Three ascending lists per query:
//   ranked   the D-pairs that are ranked per completion = allowed + live, as D-pair indices;
//   allowed  the hero hands whose class is in hero_range, as SLOTS of `ranked`;
//   live     the D-pairs whose entry in the opponent's table (McqHeroKind<W>::opp_t: the range bits of mcq_exact_ext_cbits,
//            or eff_opp) is not 0 -- the only hands the opponent can ever hold, whatever hero holds: mcq_exact_ext_w2 of
//            range bits 0 is 0 --, as slots of `ranked`.
// Keys and records are kept per slot; a hero hand walks `live` only and finds its own key at its own slot, so rank and walk
// cost what the ranges leave, not 1326 x 1081.  A group of few hero hands shares each hand's walk among several threads
// (mcq_exact_hero_pre_share).
// Sums.  A hero hand's twelve sums stay 32-bit while one block owns at most MCQ_XP_MAX_OWNED completions (one completion
// adds at most 2 x 1081 to tot); the host sends the completions in slices of at most that many per launch and the rows are
// accumulated across launches with 64-bit integer atomics.
// Weighted hands (McqHeroKind<true>: mcq_exact_hero_pre_w_kernel): the same lists made from the two weight tables per
// D-pair, the weight in the record, 64-bit sums per thread -- see "weighted hands" below for what that changes.
#ifndef MCQ_EXACT_HERO_PRE_HPP
#define MCQ_EXACT_HERO_PRE_HPP

#include "mcq_exact_hero.hpp"

#define MCQ_XP_MAX_D 52u        /* |D|: before the flop, no ghost cards */
#define MCQ_XP_MAX_PAIRS 1326u  /* C(52, 2) D-pairs = hero hands = MCQ_XH_ROWS */
#define MCQ_XP_MAX_CAND 1081u   /* C(47, 2) hands that a completion leaves alive */
#define MCQ_XP_MAX_BOARDS 2598960u /* C(52, 5) */
#define MCQ_XP_MAX_OWNED 1500000u  /* completions whose sums one thread may keep in 32 bits */
#define MCQ_XP_DEFAULT_SLICE 262144u /* completions per launch: ten launches for C(52, 5) */

static_assert(MCQ_XP_MAX_PAIRS == MCQ_XH_ROWS, "one row per D-pair of the full deck");
static_assert(MCQ_XP_MAX_PAIRS > MCQ_XX_MAX_RP && MCQ_XP_MAX_D > MCQ_XX_MAX_L,
              "mcq_exact_ext.hpp's sizes (50 cards, 1225 pairs) do not cover |D| = 52: this header sizes its own arrays");
static_assert((MCQ_XP_MAX_D - 5u) * (MCQ_XP_MAX_D - 6u) / 2u == MCQ_XP_MAX_CAND, "hands left by a completion");
static_assert((uint64_t)MCQ_XP_MAX_OWNED * 2u * MCQ_XP_MAX_CAND < (1ull << 32), "a hero hand's sums of one launch fit 32 bits");
static_assert(MCQ_XP_DEFAULT_SLICE <= MCQ_XP_MAX_OWNED, "the default slice keeps that bound whatever the grid");
static_assert(MCQ_XP_MAX_D - 1u < 64u, "D-positions fit the 6-bit fields of mcq_exact_ext_pack");
/* mcq_exact_binom and mcq_exact_unrank say "n <= 50"; at L = 52, k = 5 their intermediates still fit 32 bits: the largest
 * binomial met is C(51, 5) = 2 349 060, and it is multiplied by at most 51 before the exact division. */
static_assert(2349060ull * 51ull < (1ull << 32), "mcq_exact_unrank at L = 52, k = 5");

// The query of a record with ANY number of table cards is mcq_exact_hero_query without need_flop.

// The three lists, one D-pair after the other (the kernel makes the same lists with ballots); opp_tab from
// mcq_exact_ext_cb_table or ow_tab, hw_tab for W = true only, MCQ_XP_MAX_PAIRS entries each.  n[0..3) = allowed, live,
// ranked.  (Host planning counts `allowed` by mcq_exact_hero_count, from the same predicate: host and every block agree.)
template <bool W>
MCQ_HD void mcq_exact_hero_pre_lists(const McqExactHeroQuery &e, const uint8_t *r_id, const typename McqHeroKind<W>::opp_t *opp_tab,
                                     const uint16_t *hw_tab, uint16_t *allowed, uint16_t *live, uint16_t *ranked, uint32_t n[3]) {
    n[0] = n[1] = n[2] = 0u;
    uint32_t rp = 0;
    for (uint32_t qb = 1; qb < e.x.b.L; qb++)
        for (uint32_t qa = 0; qa < qb; qa++, rp++) {
            const bool is_allowed = McqHeroKind<W>::allowed(e, r_id, hw_tab, rp, qa, qb), is_live = opp_tab[rp] != 0u;
            if (!is_allowed && !is_live) continue;
            if (is_allowed) allowed[n[0]++] = (uint16_t)n[2];
            if (is_live) live[n[1]++] = (uint16_t)n[2];
            ranked[n[2]++] = (uint16_t)rp;
        }
}

// the D-positions of a completion's table cards as a mask
MCQ_HD uint64_t mcq_exact_hero_pre_mask(const McqExactQuery &b, const uint32_t pos[5]) {
    uint64_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++)
        if (i < b.k) m |= 1ull << pos[i];
    return m;
}

// The completion that follows pos[0..k) (ascending D-positions) in the order of mcq_exact_unrank's index: a block unranks
// the first completion of its share once and steps from there -- scalar work of a few instructions where unranking walks
// down the deck with a division per step.  Unused entries (i >= k) stay 255.
MCQ_HD void mcq_exact_hero_pre_next(uint32_t pos[5], uint32_t k) {
    bool carry = true;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++)
        if (i < k && carry) {
            if (i + 1u < k && pos[i] + 1u == pos[i + 1u < 5u ? i + 1u : 4u]) {
                pos[i] = i; /* the lowest cards start over */
            } else {
                pos[i]++;
                carry = false;
            }
        }
}

// Ranking pass, lane `lane` of `n_lanes`: key and packed record (McqHeroKind<W>::pack) of the slots lane, lane + n_lanes,
// ... of `ranked` (pair_xy[rp] = qa | qb << 8, d_card[p] = mcq_card(r_id[p]), taken = mcq_exact_hero_pre_mask).
template <bool W>
MCQ_HD void mcq_exact_hero_pre_rank(const McqExactHeroQuery &e, const McqExactBoard &bd, uint64_t taken, uint32_t lane,
                                    uint32_t n_lanes, const uint16_t *ranked, uint32_t n_ranked, const uint16_t *pair_xy,
                                    const McqCard *d_card, const typename McqHeroKind<W>::opp_t *opp_tab, const uint32_t *tf,
                                    const uint32_t *tops, const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    for (uint32_t i = lane; i < n_ranked; i += n_lanes) {
        const uint32_t rp = ranked[i], xy = pair_xy[rp], pa = xy & 0xFFu, pb = xy >> 8;
        uint32_t key = 0u, r = 0u; /* dead: a table card took one of its cards */
        if ((((taken >> pa) | (taken >> pb)) & 1ull) == 0ull) {
            McqHole h;
            h.set(d_card[pa], d_card[pb]);
            key = mcq_eval_key(bd.b, bd.fs, h, tf, tops, sd);
            r = McqHeroKind<W>::pack(pa, pb, bd.top, e.x.b.k != 0u, opp_tab[rp]);
        }
        keys[i] = key;
        rec[i] = r;
    }
}

// A group of blocks owns n_g <= 1024 hero hands.  Where they leave threads idle, `share` threads walk for ONE hero hand,
// thread `sub` of them the live hands sub, sub + share, ...: a narrow hero range would otherwise leave its walk to a
// single wave, one step after the other.  Each thread keeps its own sums; they meet in the row's atomics.
MCQ_HD uint32_t mcq_exact_hero_pre_share(uint32_t n_g) {
    const uint32_t s = 1024u / (n_g ? n_g : 1u);
    return s > 64u ? 64u : s < 1u ? 1u : s;
}

// The class-bit walk of ONE hero hand h = D-positions qa < qb at slot `own` (keys[own] != 0: the completion left it alive):
// the live hands j0, j0 + step, ... as the opponent's (a dead one: record 0, weight 0).  A loop of its own beside
// mcq_exact_hero_walk_as: through that one it was measured 0.2 to 2.8 % FASTER on the two larger shapes under both laws,
// below what the same code gives against itself (profiles/hero_refactor_ab.txt, "discarded variants") -- a loop that the
// compiler laid out anew, whose other shapes nobody has measured.  Returns the hero hand's type.
MCQ_HD uint32_t mcq_exact_hero_pre_walk_bits(const bool ref, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t own,
                                             const uint16_t *live, uint32_t n_live, uint32_t j0, uint32_t step, const uint32_t *keys,
                                             const uint32_t *rec, McqExactAcc &acc) {
    const uint32_t kh = keys[own], ah = mcq_exact_ext_above(rec[own]);
    for (uint32_t j = j0; j < n_live; j += step) {
        const uint32_t s = live[j], r = rec[s], pa = r & 63u, pb = (r >> 6) & 63u;
        const bool shared = pa == qa || pa == qb || pb == qa || pb == qb; /* (hero's own hand among them) */
        const bool ok = !shared && (!ref || ah + mcq_exact_ext_above(r) < bd.u);
        const uint32_t w = ok ? mcq_exact_ext_w2(ref, mcq_exact_ext_cb(r), pa, pb, qa, qb) : 0u;
        const uint32_t kj = keys[s];
        acc.win += kj < kh ? w : 0u;
        acc.tie += kj == kh ? w : 0u;
        acc.tot += w;
    }
    return mcq_key_type(kh);
}

// The walk of one hero hand, with the commonest stride (1: a group of more than 512 hands) and, W = false, the law as
// constants of two or four copies of the loop (W = true: mcq_exact_hero_walk_as over `live`, the uniform law only).
template <bool W>
MCQ_HD uint32_t mcq_exact_hero_pre_walk(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t own,
                                        const uint16_t *live, uint32_t n_live, uint32_t j0, uint32_t step, const uint32_t *keys,
                                        const uint32_t *rec, McqExactAcc &acc) {
    if constexpr (W) {
        return step == 1u ? mcq_exact_hero_walk_as<W, true>(false, bd.u, qa, qb, own, live, n_live, j0, 1u, keys, rec, acc)
                          : mcq_exact_hero_walk_as<W, true>(false, bd.u, qa, qb, own, live, n_live, j0, step, keys, rec, acc);
    } else {
        if (e.x.b.ref_law)
            return step == 1u ? mcq_exact_hero_pre_walk_bits(true, bd, qa, qb, own, live, n_live, j0, 1u, keys, rec, acc)
                              : mcq_exact_hero_pre_walk_bits(true, bd, qa, qb, own, live, n_live, j0, step, keys, rec, acc);
        return step == 1u ? mcq_exact_hero_pre_walk_bits(false, bd, qa, qb, own, live, n_live, j0, 1u, keys, rec, acc)
                          : mcq_exact_hero_pre_walk_bits(false, bd, qa, qb, own, live, n_live, j0, step, keys, rec, acc);
    }
}

// ---------------------------------------------------------------------------------------------- weighted hands
// mcq_exact_batch_hero_range_preflop_weighted: mcq_exact_hero.hpp's McqHeroKind<true> on D-pairs.  What differs from the
// above: a ranked slot's record is mcq_exact_hero_w_pack(pa, pb, eff_opp); a pair that a table card touches keeps key 0 and
// record 0, whose weight is 0.
// Sums.  A thread's sums of ONE completion stay 32-bit (McqExactAcc) whatever its share of the walk; they are added once
// per completion into McqHeroKind<true>::Sums (64-bit), so MCQ_XP_MAX_OWNED bounds nothing here -- plan and slices are kept
// only so that launch lengths and grids stay what callers know.
static_assert(MCQ_XP_MAX_CAND * MCQ_XH_WEIGHT_MAX < (1u << 27), "a completion's weighted sums (McqExactAcc) fit 32 bits");
static_assert((uint64_t)MCQ_XP_MAX_OWNED * MCQ_XP_MAX_CAND * MCQ_XH_WEIGHT_MAX > 0xFFFFFFFFull,
              "a thread's weighted sums of one launch do NOT fit 32 bits: McqHeroKind<true>::Sums is 64-bit");
static_assert((uint64_t)MCQ_XP_MAX_BOARDS * MCQ_XP_MAX_CAND * MCQ_XH_WEIGHT_MAX < (1ull << 48),
              "... and 64 bits hold a hero hand's sums over all C(52, 5) completions with room");

// ---- host side
// Is some opponent hand of positive weight left against EVERY allowed hero hand?  Exact whatever k: a live D-pair g that
// shares no card with h leaves |D| - 4 >= k cards, so a completion that avoids both exists and h's row gets weight; without
// such a g it gets none.  One pass over allowed x live D-pairs, at most 1326^2 steps, before anything is launched.
// -> MCQ_XP_MAX_PAIRS if so, else the D-pair index of the first hero hand left without an opponent.
MCQ_HD uint32_t mcq_exact_hero_pre_w_undealable(const McqExactHeroQuery &e, const uint16_t *ow_tab, const uint16_t *hw_tab) {
    uint32_t rp = 0;
    for (uint32_t qb = 1; qb < e.x.b.L; qb++)
        for (uint32_t qa = 0; qa < qb; qa++, rp++) {
            if (hw_tab[rp] == 0u) continue;
            bool found = false;
            uint32_t g = 0;
            for (uint32_t pb = 1; pb < e.x.b.L && !found; pb++)
                for (uint32_t pa = 0; pa < pb; pa++, g++)
                    if (ow_tab[g] != 0u && pa != qa && pa != qb && pb != qa && pb != qb) {
                        found = true;
                        break;
                    }
            if (!found) return rp;
        }
    return MCQ_XP_MAX_PAIRS;
}

// The completions go out in launches of `slice`; a launch's grid gives every group of blocks `per` blocks, each of which
// owns a run of consecutive completions of this length (the last ones fewer) -- the plan is sound iff it is at most
// MCQ_XP_MAX_OWNED.
MCQ_HD uint32_t mcq_exact_hero_pre_owned(uint32_t slice, uint32_t per) { return (slice + per - 1u) / per; }

// clamps a requested slice (0: the default) to what the 32-bit sums allow with a single block per group
MCQ_HD uint32_t mcq_exact_hero_pre_slice(uint64_t want) {
    if (want == 0u) return MCQ_XP_DEFAULT_SLICE;
    return want > MCQ_XP_MAX_OWNED ? MCQ_XP_MAX_OWNED : (uint32_t)want;
}

// ---- the two preflop entries by name
// mcq_exact_batch_hero_range_preflop (_pre) and ..._preflop_weighted (_pre_w) as fixed instances of the code above, as in
// mcq_exact_hero.hpp: the names the host builds of the tests walk an entry through.
MCQ_HD int mcq_exact_hero_pre_query(const McqQueryWords &q, const McqExtRec &er, int law, McqExactHeroQuery &e) {
    return mcq_exact_hero_query(q, er, law, false, e);
}
MCQ_HD void mcq_exact_hero_pre_lists(const McqExactHeroQuery &e, const uint8_t *r_id, const uint8_t *cb_tab, uint16_t *allowed,
                                     uint16_t *live, uint16_t *ranked, uint32_t n[3]) {
    mcq_exact_hero_pre_lists<false>(e, r_id, cb_tab, nullptr, allowed, live, ranked, n);
}
MCQ_HD void mcq_exact_hero_pre_w_lists(const McqExactHeroQuery &e, const uint16_t *ow_tab, const uint16_t *hw_tab, uint16_t *allowed,
                                       uint16_t *live, uint16_t *ranked, uint32_t n[3]) {
    mcq_exact_hero_pre_lists<true>(e, nullptr, ow_tab, hw_tab, allowed, live, ranked, n);
}
MCQ_HD void mcq_exact_hero_pre_rank(const McqExactHeroQuery &e, const McqExactBoard &bd, uint64_t taken, uint32_t lane,
                                    uint32_t n_lanes, const uint16_t *ranked, uint32_t n_ranked, const uint16_t *pair_xy,
                                    const McqCard *d_card, const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops,
                                    const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    mcq_exact_hero_pre_rank<false>(e, bd, taken, lane, n_lanes, ranked, n_ranked, pair_xy, d_card, cb_tab, tf, tops, sd, keys, rec);
}
MCQ_HD uint32_t mcq_exact_hero_pre_walk(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t own,
                                        const uint16_t *live, uint32_t n_live, uint32_t j0, uint32_t step, const uint32_t *keys,
                                        const uint32_t *rec, McqExactAcc &acc) {
    return mcq_exact_hero_pre_walk<false>(e, bd, qa, qb, own, live, n_live, j0, step, keys, rec, acc);
}
/* (a weighted record packs nothing of the query and the uniform law asks nothing of the completion) */
MCQ_HD void mcq_exact_hero_pre_w_rank(const McqExactBoard &bd, uint64_t taken, uint32_t lane, uint32_t n_lanes, const uint16_t *ranked,
                                      uint32_t n_ranked, const uint16_t *pair_xy, const McqCard *d_card, const uint16_t *ow_tab,
                                      const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    const McqExactHeroQuery e = McqExactHeroQuery();
    mcq_exact_hero_pre_rank<true>(e, bd, taken, lane, n_lanes, ranked, n_ranked, pair_xy, d_card, ow_tab, tf, tops, sd, keys, rec);
}
MCQ_HD uint32_t mcq_exact_hero_pre_w_walk(uint32_t qa, uint32_t qb, uint32_t own, const uint16_t *live, uint32_t n_live, uint32_t j0,
                                          uint32_t step, const uint32_t *keys, const uint32_t *rec, McqExactAcc &acc) {
    const McqExactHeroQuery e = McqExactHeroQuery();
    const McqExactBoard bd = McqExactBoard();
    return mcq_exact_hero_pre_walk<true>(e, bd, qa, qb, own, live, n_live, j0, step, keys, rec, acc);
}

#endif /* MCQ_EXACT_HERO_PRE_HPP */
