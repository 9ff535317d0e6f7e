// mcq_exact_hero.hpp -- exact enumeration with the HERO given as a range: every hero hand against one random opponent
// (ranged or not) from ONE enumeration; lane code shared by mcq_exact_hero_kernel and mcq_exact_hero_w_kernel
// (mcq_kernels.hip) and the host builds of the tests (tests/hostsim_hero_range, tests/hostsim_hero_weighted).  The pieces of
// mcq_exact.hpp and mcq_exact_ext.hpp are reused unchanged.
//
// What is enumerated.  D = 52 cards minus table and ghost, ascending card id; Ld = |D| <= 49 (postflop).  Positions run
// over D.  A hero hand h = D-positions qa < qb (index qb (qb - 1) / 2 + qa, up to C(49, 2) = 1176 of them) is fixed
// across the table completions; the completions are the k-subsets of D (k = 5 - n_board <= 2), and the m = Ld - k <= 47
// cards left hold C(m, 2) <= 1081 candidate hands, each of which is somebody's hero hand AND everybody else's
// opponent hand: they are ranked ONCE per completion.
// Row of hero hand h = what mcq_exact_ext.hpp makes of the record whose hero holds h: its deck R is D minus h, so
//   * the completions of R are the completions of D that miss h;
//   * the opponent's hand {pa < pb}, disjoint from h, has the weight of a SECOND hand once the first hand h has left the
//     deck (mcq_exact_ext_w2: prev(pb) skips hero's cards) -- under MCQ_LAW_UNIFORM cls(pa, pb);
//   * MCQ_LAW_REFERENCE: a completion T is possible iff some card of R above max(T) is not in the opponent's hand, i.e.
//     above(h) + above(opponent) < the cards of D above max(T)        (as the two-opponent pass B counts it).
// The sums of a hero hand are integers: win = weight of the opponent hands strictly below, tie = level, runs = all.
// The hero's own draw (the aggregate): MCQ_LAW_REFERENCE accepts the ordered pairs (A, B) of D with B not D's highest
// card and the hand leaves by value (montecarlo_python.py:136-148), so hand {a < b} is dealt 2 - [b is D's top] times
// in proportion; MCQ_LAW_UNIFORM deals every allowed hand equally often.
#ifndef MCQ_EXACT_HERO_HPP
#define MCQ_EXACT_HERO_HPP

#include "mcq_exact_ext.hpp"

#define MCQ_XH_MAX_D 49u       /* |D|: the flop, no ghost cards */
#define MCQ_XH_MAX_HANDS 1176u /* C(49, 2) hero hands */
#define MCQ_XH_MAX_PAIRS 1081u /* C(47, 2) candidate hands of a completion */
#define MCQ_XH_ROWS 1326u      /* C(52, 2) = MCQ_HAND_ROWS: row of hand {a < b} = b (b - 1) / 2 + a */
#define MCQ_XH_SUMS 12u        /* per hero hand: win, tie, tot, by_type[9] */

static_assert(MCQ_XH_MAX_PAIRS > MCQ_EXACT_PAIRS, "a hero range leaves 47 cards, not 45: size the arrays for 1081 hands");
static_assert(MCQ_XH_MAX_HANDS <= MCQ_XX_MAX_RP, "the range-bit table of mcq_exact_ext_cb_table holds every D-pair");
static_assert(MCQ_XH_MAX_HANDS * 2u * MCQ_EXACT_PAIRS < (1u << 22), "a hero hand's sums fit 32 bits");

/* why a record cannot be enumerated (0 = it can) */
#define MCQ_XH_OK 0
#define MCQ_XH_INVALID 1    /* what mcq_eval_batch_ext refuses */
#define MCQ_XH_NOT_RANGE 2  /* hero_is_range == 0 */
#define MCQ_XH_KNOWN 3      /* n_known != 0 */
#define MCQ_XH_PLAYERS 4    /* n_players != 2 */
#define MCQ_XH_PREFLOP 5    /* fewer than three table cards */
#define MCQ_XH_EMPTY 6      /* no allowed hero hand in D */
#define MCQ_XH_UNDEALABLE 7 /* an allowed hero hand against which the opponent's range cannot be dealt (a row's runs == 0) */

struct McqExactHeroQuery { /* wave-uniform */
    McqExactExtQuery x;    /* b.deck = D, b.L = |D|, k, law, table cards; m, n_pairs, n_rp = C(|D|, 2); the opponent's range */
    uint32_t hero_bits[6]; /* the hero's range */
    uint32_t n_allowed;    /* hero hands in D whose class is in it (host side: mcq_exact_hero_count) */
};

MCQ_HD bool mcq_exact_hero_allowed(const McqExactHeroQuery &e, const uint8_t *r_id, uint32_t qa, uint32_t qb) {
    return mcq_in_range(e.hero_bits, r_id[qa], r_id[qb]);
}

// need_flop: refuse a record with fewer than three table cards (the postflop entries; mcq_exact_hero_pre.hpp takes any
// number).  The refusals are tested in the order of their codes.
MCQ_HD int mcq_exact_hero_query(const McqQueryWords &q, const McqExtRec &er, int law, bool need_flop, McqExactHeroQuery &e) {
    if (!mcq_query_ext_valid(q, er)) return MCQ_XH_INVALID;
    if (!er.hero_is_range()) return MCQ_XH_NOT_RANGE;
    if (er.n_known() != 0u) return MCQ_XH_KNOWN;
    if (q.n_players() != 2u) return MCQ_XH_PLAYERS;
    if (need_flop && q.n_board() < 3u) return MCQ_XH_PREFLOP;
    const uint64_t deck = mcq_ext_base_deck(q, er);
    McqExactExtQuery &x = e.x;
    x.n_known = 0u;
    for (uint32_t h = 0; h < MCQ_MAX_KNOWN; h++) x.known[h] = 0u;
    x.b.deck_lo = (uint32_t)deck;
    x.b.deck_hi = (uint32_t)(deck >> 32);
    x.b.L = mcq_popc(x.b.deck_lo) + mcq_popc(x.b.deck_hi);
    x.b.k = 5u - q.n_board();
    x.b.n_opp = 1u;
    x.b.ref_law = law == MCQ_LAW_REFERENCE;
    x.b.known.clear();
    for (uint32_t i = 0; i < q.n_board(); i++) x.b.known.add(mcq_card(q.card(2u + i)));
    x.b.hero.set(mcq_card(0u), mcq_card(1u)); /* (nobody's: every hero hand comes from the candidates) */
    x.m = x.b.L - x.b.k;
    x.n_pairs = x.m * (x.m - 1u) / 2u;
    x.n_rp = x.b.L * (x.b.L - 1u) / 2u;
    x.ranged = !mcq_ext_opp_all(er);
    for (uint32_t i = 0; i < 6; i++) {
        x.bits[i] = er.w[er.opp_set() + i];
        e.hero_bits[i] = er.w[er.hero_set() + i];
    }
    e.n_allowed = 0u; /* the host counts them: mcq_exact_hero_count */
    return MCQ_XH_OK;
}

// One table completion without a hero: pos[0..k) ascending D-positions of the new table cards (mcq_exact_board's
// table, flush selector, top and u; hero_key stays 0).
MCQ_HD void mcq_exact_hero_board(const McqExactQuery &e, const uint32_t pos[5], const uint8_t *r_id, McqExactBoard &o) {
    o.b = e.known;
    o.top = 0;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++)
        if (i < e.k) {
            o.b.add(mcq_card(r_id[pos[i]]));
            o.top = pos[i]; /* ascending: the last one is the highest */
        }
    o.fs.from_board(o.b);
    o.hero_key = 0u;
    o.u = e.k ? e.L - 1u - o.top : 64u; /* nothing to draw: nothing is excluded */
}

// row of the hero hand at D-positions qa < qb
MCQ_HD uint32_t mcq_exact_hero_row(const uint8_t *r_id, uint32_t qa, uint32_t qb) {
    const uint32_t a = r_id[qa], b = r_id[qb];
    return b * (b - 1u) / 2u + a;
}

// ---------------------------------------------------------------------------------------------- class bits or a weight per hand
// The four entries differ in ONE compile-time switch.  W = false: a hand counts by the class bit of its range, under either
// law.  W = true (mcq_exact_batch_hero_range_weighted, ..._preflop_weighted): an integer weight per HAND in place of the
// class bit, MCQ_LAW_UNIFORM only -- the reference's law tests the class of the drawn index pair and deals "the card after
// B", a weight per dealt hand has no meaning there, so McqHeroKind<true> does not name its terms and they are not compiled
// in.  Both ranges keep their class sets; the tables are indexed by row (mcq_exact_hero_row) and folded once into tables per
// D-pair (mcq_exact_hero_w_tables):
//   ow_tab[rp] = eff_opp  = opp_w[row]                 if the pair's class is in the opponent's range, else 0
//   hw_tab[rp] = eff_hero = hero_w ? hero_w[row] : 1   if the pair's class is in the hero's range,     else 0
// What a kind carries:
//   Sums     a hero hand's sums over all completions, 32- or 64-bit (the static_asserts below);
//   opp_t    the opponent's table per D-pair: the range bits (mcq_exact_ext_cb_table, mcq_exact_ext_cbits) or ow_tab.  A
//            D-pair is LIVE -- the opponent can hold it at all -- iff its entry is not 0, under both kinds;
//   allowed  is the D-pair a hero hand?  the class is in hero_range, or eff_hero > 0 (host and kernel alike);
//   pack     the record of a ranked candidate: mcq_exact_ext_pack, or positions and eff_opp in the 16 bits above them (the
//            `above` and range-bit fields are not needed under the uniform law);
//   law_ok,  W = true only, for the one walk loop of the two weighted entries (mcq_exact_hero_walk_as): no law test, the
//   weight   weight one shift.  The class-bit walks -- mcq_exact_ext_w2 under the law test ah + above(r) < u -- keep a
//            loop per street, mcq_exact_hero_walk<false> and mcq_exact_hero_pre_walk_bits: see there.
#define MCQ_XH_WEIGHT_MAX 65535u /* MCQ_COMBO_WEIGHT_MAX */

static_assert(MCQ_XH_MAX_PAIRS * MCQ_XH_WEIGHT_MAX < (1u << 27), "a completion's weighted sums (McqExactAcc) fit 32 bits");
static_assert((uint64_t)MCQ_XH_MAX_PAIRS * MCQ_EXACT_PAIRS * MCQ_XH_WEIGHT_MAX > 0xFFFFFFFFull,
              "a hero hand's weighted sums over the flop's 1081 completions do NOT fit 32 bits: McqHeroKind<true>::Sums is 64-bit");
static_assert((uint64_t)MCQ_XH_MAX_HANDS * MCQ_XH_MAX_PAIRS * MCQ_XH_WEIGHT_MAX < (1ull << 37), "... and 64 bits hold them with room");

template <class T>
struct McqHeroSums { /* a hero hand's sums over all completions */
    T win, tie, tot, type[9];
};

// packed record of a candidate hand under W = true: D-positions, eff_opp
MCQ_HD uint32_t mcq_exact_hero_w_pack(uint32_t pa, uint32_t pb, uint32_t w) { return pa | (pb << 6) | (w << 16); }

template <bool W>
struct McqHeroKind;

template <>
struct McqHeroKind<false> {
    typedef McqHeroSums<uint32_t> Sums; /* see the static_assert on MCQ_XH_MAX_HANDS above */
    typedef uint8_t opp_t;
    static MCQ_HDM bool allowed(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *, uint32_t, uint32_t qa, uint32_t qb) {
        return mcq_exact_hero_allowed(e, r_id, qa, qb);
    }
    static MCQ_HDM uint32_t pack(uint32_t pa, uint32_t pb, uint32_t top, bool drawn, uint32_t cb) {
        return mcq_exact_ext_pack(pa, pb, top, drawn, cb);
    }
};

template <>
struct McqHeroKind<true> {
    typedef McqHeroSums<unsigned long long> Sums; /* see the static_asserts above */
    typedef uint16_t opp_t;
    static MCQ_HDM bool allowed(const McqExactHeroQuery &, const uint8_t *, const uint16_t *hw_tab, uint32_t rp, uint32_t, uint32_t) {
        return hw_tab[rp] != 0u;
    }
    static MCQ_HDM uint32_t pack(uint32_t pa, uint32_t pb, uint32_t, bool, uint32_t w) { return mcq_exact_hero_w_pack(pa, pb, w); }
    static MCQ_HDM uint32_t above(uint32_t) { return 0u; }
    static MCQ_HDM bool law_ok(const bool, uint32_t, uint32_t, uint32_t) { return true; }
    static MCQ_HDM uint32_t weight(const bool, uint32_t r, uint32_t, uint32_t, uint32_t, uint32_t) { return r >> 16; }
};

// the two tables per D-pair; entries rp0, rp0 + step, ...
MCQ_HD void mcq_exact_hero_w_tables(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *opp_w, const uint16_t *hero_w,
                                    uint32_t rp0, uint32_t step, uint16_t *ow_tab, uint16_t *hw_tab) {
    for (uint32_t rp = rp0; rp < e.x.n_rp; rp += step) {
        uint32_t pa, pb;
        mcq_exact_pair_xy(rp, pa, pb);
        const uint32_t row = mcq_exact_hero_row(r_id, pa, pb);
        ow_tab[rp] = mcq_in_range(e.x.bits, r_id[pa], r_id[pb]) ? opp_w[row] : (uint16_t)0u;
        hw_tab[rp] = mcq_in_range(e.hero_bits, r_id[pa], r_id[pb]) ? (hero_w ? hero_w[row] : (uint16_t)1u) : (uint16_t)0u;
    }
}

// The allowed hero hands as D-pair indices, ascending -> their number (hw_tab: W = true only).  (The kernel makes the same
// list with ballots.)
template <bool W>
MCQ_HD uint32_t mcq_exact_hero_count(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *hw_tab, uint16_t *list) {
    uint32_t n = 0;
    for (uint32_t rp = 0; rp < e.x.n_rp; rp++) {
        uint32_t qa, qb;
        mcq_exact_pair_xy(rp, qa, qb);
        if (!McqHeroKind<W>::allowed(e, r_id, hw_tab, rp, qa, qb)) continue;
        if (list) list[n] = (uint16_t)rp;
        n++;
    }
    return n;
}

// Ranking pass, lane `lane` of `n_lanes`: key and packed record (McqHeroKind<W>::pack) of the candidate hands lane,
// lane + n_lanes, ... of this completion.
template <bool W>
MCQ_HD void mcq_exact_hero_rank(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t lane, uint32_t n_lanes,
                                const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos,
                                const typename McqHeroKind<W>::opp_t *opp_tab, const uint32_t *tf, const uint32_t *tops,
                                const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    for (uint32_t i = lane; i < e.x.n_pairs; i += n_lanes) {
        const uint32_t xy = pair_xy[i], x = xy & 0xFFu, y = xy >> 8;
        McqHole h;
        h.set(rem_card[x], rem_card[y]);
        keys[i] = mcq_eval_key(bd.b, bd.fs, h, tf, tops, sd);
        const uint32_t pa = rem_pos[x], pb = rem_pos[y];
        rec[i] = McqHeroKind<W>::pack(pa, pb, bd.top, e.x.b.k != 0u, opp_tab[pb * (pb - 1u) / 2u + pa]);
    }
}

// The walk of ONE hero hand h = D-positions qa < qb, whose key and record wait at index `own`: the hands j0, j0 + step, ...
// below n -- LIST: of the list `via` (mcq_exact_hero_pre.hpp), else of keys and records themselves -- as the opponent's.
// u = the completion's.  A completion's sums stay 32-bit under both kinds.  Returns the hero hand's type.
// Written on McqHeroKind<W>, instantiated for W = true alone: with W = false both streets' kernels came out of the compiler
// with the law test and the weight in another order and their call times outside what the same code gives against
// itself (profiles/hero_refactor_ab.txt), so those two walks are loops of their own.
template <bool W, bool LIST>
MCQ_HD uint32_t mcq_exact_hero_walk_as(const bool ref, uint32_t u, uint32_t qa, uint32_t qb, uint32_t own, const uint16_t *via, uint32_t n,
                                       uint32_t j0, uint32_t step, const uint32_t *keys, const uint32_t *rec, McqExactAcc &acc) {
    static_assert(W, "the class-bit walks are mcq_exact_hero_walk<false> and mcq_exact_hero_pre_walk_bits");
    const uint32_t kh = keys[own], ah = McqHeroKind<W>::above(rec[own]);
    for (uint32_t j = j0; j < n; j += step) {
        const uint32_t s = LIST ? via[j] : j, r = rec[s], pa = r & 63u, pb = (r >> 6) & 63u;
        const bool shared = pa == qa || pa == qb || pb == qa || pb == qb; /* (hero's own hand among them) */
        const bool ok = !shared && McqHeroKind<W>::law_ok(ref, ah, u, r);
        const uint32_t w = ok ? McqHeroKind<W>::weight(ref, r, pa, pb, qa, qb) : 0u;
        const uint32_t kj = keys[s];
        acc.win += kj < kh ? w : 0u;
        acc.tie += kj == kh ? w : 0u;
        acc.tot += w;
    }
    return mcq_key_type(kh);
}

// ... of candidate mi of this completion (mcq_exact_ext_m_index): every candidate hand as the opponent's.  (The law is read
// from the query: no copy of the loop per law.)
// W = false keeps a loop of its own: through mcq_exact_hero_walk_as it was measured 2 to 3 % faster with every hand on
// both sides but half a percent slower with 25 % ranges on the flop, outside what the same code gives against itself
// (profiles/hero_refactor_ab.txt, "discarded variants").
template <bool W>
MCQ_HD uint32_t mcq_exact_hero_walk(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t mi,
                                    const uint32_t *keys, const uint32_t *rec, McqExactAcc &acc) {
    if constexpr (W) {
        return mcq_exact_hero_walk_as<W, false>(false, bd.u, qa, qb, mi, nullptr, e.x.n_pairs, 0u, 1u, keys, rec, acc);
    } else {
        const uint32_t kh = keys[mi], ah = mcq_exact_ext_above(rec[mi]);
        const bool ref = e.x.b.ref_law;
        for (uint32_t j = 0; j < e.x.n_pairs; j++) {
            const uint32_t r = rec[j], pa = r & 63u, pb = (r >> 6) & 63u;
            const bool shared = pa == qa || pa == qb || pb == qa || pb == qb; /* (hero's own hand among them) */
            const bool ok = !shared && (!ref || ah + mcq_exact_ext_above(r) < bd.u);
            const uint32_t w = ok ? mcq_exact_ext_w2(ref, mcq_exact_ext_cb(r), pa, pb, qa, qb) : 0u;
            const uint32_t kj = keys[j];
            acc.win += kj < kh ? w : 0u;
            acc.tie += kj == kh ? w : 0u;
            acc.tot += w;
        }
        return mcq_key_type(kh);
    }
}

template <class T>
MCQ_HD void mcq_exact_hero_add(McqHeroSums<T> &s, const McqExactAcc &a, uint32_t type) { /* once per completion */
    s.win += a.win;
    s.tie += a.tie;
    s.tot += a.tot;
#pragma unroll
    for (uint32_t t = 0; t < 9; t++) s.type[t] += t == type ? a.win + a.tie : 0u;
}

// ---- host side
// how often the law deals hero the hand at D-positions qa < qb, in proportion
MCQ_HD uint32_t mcq_exact_hero_weight(const McqExactHeroQuery &e, uint32_t qb) {
    return e.x.b.ref_law ? (qb + 1u == e.x.b.L ? 1u : 2u) : 1u;
}

// The aggregate of one query from its MCQ_XH_ROWS rows: the allowed rows combined in ascending row order, each with the
// law's weight (hw_tab == null) or with eff_hero.  false: an allowed row has no weight -- the opponent's range cannot be
// dealt against that hand (p is then left alone).
MCQ_HD bool mcq_exact_hero_finish(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *hw_tab, const mcq_result *rows,
                                  mcq_exact_prob &p) {
    uint8_t pos_of[52];
    for (uint32_t c = 0; c < 52; c++) pos_of[c] = 255;
    for (uint32_t i = 0; i < e.x.b.L; i++) pos_of[r_id[i]] = (uint8_t)i;
    double num[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, den = 0;
    for (uint32_t b = 1; b < 52; b++)
        for (uint32_t a = 0; a < b; a++) {
            const uint32_t qa = pos_of[a], qb = pos_of[b];
            if (qa == 255u || qb == 255u) continue;
            const uint32_t hw = hw_tab ? hw_tab[qb * (qb - 1u) / 2u + qa]
                                       : (mcq_exact_hero_allowed(e, r_id, qa, qb) ? mcq_exact_hero_weight(e, qb) : 0u);
            if (hw == 0u) continue;
            const mcq_result &r = rows[b * (b - 1u) / 2u + a];
            if (r.runs == 0) return false;
            const double w = (double)hw, runs = (double)r.runs;
            num[0] += w * (double)r.win / runs;
            num[1] += w * (double)r.tie / runs;
            for (uint32_t t = 0; t < 9; t++) num[2 + t] += w * (double)r.by_type[t] / runs;
            den += w;
        }
    p.win = num[0] / den;
    p.tie = num[1] / den;
    for (uint32_t t = 0; t < 9; t++) p.by_type[t] = num[2 + t] / den;
    return true;
}

// ---- the two postflop entries by name
// What mcq_exact_batch_hero_range (no suffix) and ..._weighted (_w) are made of, each a fixed instance of the code above:
// the host builds of the tests walk an entry through these names, so they need not know how the four entries share code.
typedef McqHeroKind<false>::Sums McqExactHeroSums;
typedef McqHeroKind<true>::Sums McqExactHeroSumsW;

MCQ_HD int mcq_exact_hero_query(const McqQueryWords &q, const McqExtRec &er, int law, McqExactHeroQuery &e) {
    return mcq_exact_hero_query(q, er, law, true, e);
}
MCQ_HD uint32_t mcq_exact_hero_count(const McqExactHeroQuery &e, const uint8_t *r_id, uint16_t *list) {
    return mcq_exact_hero_count<false>(e, r_id, nullptr, list);
}
MCQ_HD uint32_t mcq_exact_hero_w_count(const McqExactHeroQuery &e, const uint16_t *hw_tab, uint16_t *list) {
    return mcq_exact_hero_count<true>(e, nullptr, hw_tab, list);
}
MCQ_HD void mcq_exact_hero_rank(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t lane, uint32_t n_lanes,
                                const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos, const uint8_t *cb_tab,
                                const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    mcq_exact_hero_rank<false>(e, bd, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd, keys, rec);
}
MCQ_HD void mcq_exact_hero_w_rank(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t lane, uint32_t n_lanes,
                                  const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos, const uint16_t *ow_tab,
                                  const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    mcq_exact_hero_rank<true>(e, bd, lane, n_lanes, pair_xy, rem_card, rem_pos, ow_tab, tf, tops, sd, keys, rec);
}
MCQ_HD uint32_t mcq_exact_hero_walk(const McqExactHeroQuery &e, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t mi,
                                    const uint32_t *keys, const uint32_t *rec, McqExactAcc &acc) {
    return mcq_exact_hero_walk<false>(e, bd, qa, qb, mi, keys, rec, acc);
}
MCQ_HD uint32_t mcq_exact_hero_w_walk(const McqExactHeroQuery &e, uint32_t qa, uint32_t qb, uint32_t mi, const uint32_t *keys,
                                      const uint32_t *rec, McqExactAcc &acc) {
    const McqExactBoard bd = McqExactBoard(); /* (the uniform law asks nothing of the completion) */
    return mcq_exact_hero_walk<true>(e, bd, qa, qb, mi, keys, rec, acc);
}
MCQ_HD void mcq_exact_hero_w_add(McqExactHeroSumsW &s, const McqExactAcc &a, uint32_t type) { mcq_exact_hero_add(s, a, type); }
MCQ_HD bool mcq_exact_hero_finish(const McqExactHeroQuery &e, const uint8_t *r_id, const mcq_result *rows, mcq_exact_prob &p) {
    return mcq_exact_hero_finish(e, r_id, nullptr, rows, p);
}
MCQ_HD bool mcq_exact_hero_w_finish(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *hw_tab, const mcq_result *rows,
                                    mcq_exact_prob &p) {
    return mcq_exact_hero_finish(e, r_id, hw_tab, rows, p);
}

#endif /* MCQ_EXACT_HERO_HPP */
