// mcq_exact_ext.hpp -- exact enumeration of EXTENDED queries (SURVEY 8f-3 x 8f-2): further known hands, ghost cards and
// an opponent range; lane code shared by mcq_exact_ext_kernel (mcq_kernels.hip) and the host build of the tests
// (tests/hostsim_exact_ext).  The plain walk's pieces (mcq_exact.hpp) are reused unchanged.
//
// Every row form (plain, split-pot, per seat, per runout) is made of the same few pieces, each stated once: the known hands
// of a completion (mcq_exact_ext_known), a completion without a random opponent (mcq_exact_ext_lone_known), the walk over the
// candidate hands (mcq_exact_ext_candidates, with three small bodies) and the word of a row that a completion's sums give
// (mcq_exact_ext_row_word, mcq_exact_ext_seats_word).
//
// What is enumerated.  R = the deck the random opponents are dealt from: 52 cards minus ghost, table, hero and the known
// hands, ascending card id (montecarlo_python.py:121-163, 206-208); L = |R|.  Table-completion-major as the plain walk:
// the k = 5 - n_board new table cards T are a k-subset of R, the m = L - k cards left hold the opponents' hands --
// m = 45 - 2 n_known - 2 (ghost), so there are C(m, 2) <= 990 candidate hands.
// Weights (positions pa < pb in the opponent's current deck; cls = the range test of two cards):
//   * MCQ_LAW_REFERENCE (montecarlo_python.py:165-181): the accepted index pairs (r1, r2) are every ordered pair of
//     deck cards (A = deck[r1], B = deck[r2]) with r1 != r2, r2 < len - 1 and cls(A, B); the hand dealt is
//     deck.pop(r1), deck.pop(r2) = {A, B} if B lies below A, else {A, the card that follows B}.  So the TESTED pair is
//     not always the DEALT pair: hand {pa, pb} is reached from (A = pb, B = pa) iff cls(pa, pb), and from
//     (A = pa, B = prev(pb)) iff prev(pb) != pa and cls(pa, prev(pb)), prev = the deck card just below pb.
//       w = cls(pa, pb) + [prev(pb) != pa] cls(pa, prev(pb))       (no range: 2, or 1 for neighbours -- mcq_exact_w1/w2)
//     The second opponent's deck is R minus the first hand: prev(pb) skips the first hand's cards.
//     Table cards are never the deck's highest card: T is possible iff some card of R above max(T) is in no hand.
//   * MCQ_LAW_UNIFORM: w = cls(pa, pb); every completion equally likely.
// One random opponent (or none): P(outcome) = weight / total weight, integers as in mcq_exact.hpp.  Two opponents: the
// second draw's normaliser N2(h1) = sum of its weights depends on the first hand h1 unless every class is allowed, so the
// sums are kept PER FIRST HAND h1 (an R-pair, index pb (pb - 1) / 2 + pa), whose total S_tot(h1) = N2(h1) x (table
// completions) is that normaliser: P = sum_h1 w1(h1) / N1 x S(h1) / S_tot(h1).
#ifndef MCQ_EXACT_EXT_HPP
#define MCQ_EXACT_EXT_HPP

#include "mcq_device.hpp"
#include "mcq_exact.hpp"

#define MCQ_XX_MAX_L 50u     /* |R|: preflop, hero only */
#define MCQ_XX_MAX_RP 1225u  /* C(50, 2) first hands */
#define MCQ_XX_SUMS 12u      /* per first hand: win, tie, tot, by_type[9] */

/* why a record cannot be enumerated (0 = it can) */
#define MCQ_XX_OK 0
#define MCQ_XX_INVALID 1     /* what mcq_eval_batch_ext refuses */
#define MCQ_XX_HERO_RANGE 2
#define MCQ_XX_KNOWN_RANGE 3
#define MCQ_XX_TOO_MANY 4    /* more than two random opponents */

struct McqExactExtQuery { /* wave-uniform */
    McqExactQuery b;      /* R, L, k, n_opp = random opponents, law, table cards, hero */
    uint32_t n_known;
    uint32_t m, n_pairs;  /* cards left after a completion, candidate hands C(m, 2) */
    uint32_t n_rp;        /* first hands C(L, 2) */
    bool ranged;          /* the opponents' range leaves out a class */
    uint32_t bits[6];     /* their range (169 bits) */
    uint32_t known[MCQ_MAX_KNOWN]; /* known hand h: card ids a | b << 8 */
};

MCQ_HD int mcq_exact_ext_query(const McqQueryWords &q, const McqExtRec &er, int law, McqExactExtQuery &e) {
    if (!mcq_query_ext_valid(q, er)) return MCQ_XX_INVALID;
    if (er.hero_is_range()) return MCQ_XX_HERO_RANGE;
    const uint32_t nk = er.n_known();
    for (uint32_t h = 0; h < nk; h++)
        if (mcq_ext_hand(q, er, h + 1u) >> 16) return MCQ_XX_KNOWN_RANGE;
    if (q.n_players() > 3u + nk) return MCQ_XX_TOO_MANY;
    uint64_t deck = mcq_ext_base_deck(q, er) & ~((1ull << q.card(0)) | (1ull << q.card(1)));
    e.n_known = nk;
    for (uint32_t h = 0; h < MCQ_MAX_KNOWN; h++) {
        const uint32_t hd = h < nk ? mcq_ext_hand(q, er, h + 1u) : 0u;
        e.known[h] = hd;
        if (h < nk) deck &= ~((1ull << (hd & 0xFFu)) | (1ull << (hd >> 8)));
    }
    e.b.deck_lo = (uint32_t)deck;
    e.b.deck_hi = (uint32_t)(deck >> 32);
    e.b.L = mcq_popc(e.b.deck_lo) + mcq_popc(e.b.deck_hi);
    e.b.k = 5u - q.n_board();
    e.b.n_opp = q.n_players() - 1u - nk;
    e.b.ref_law = law == MCQ_LAW_REFERENCE;
    e.b.known.clear();
    for (uint32_t i = 0; i < q.n_board(); i++) e.b.known.add(mcq_card(q.card(2u + i)));
    e.b.hero.set(mcq_card(q.card(0)), mcq_card(q.card(1)));
    e.m = e.b.L - e.b.k;
    e.n_pairs = e.m * (e.m - 1u) / 2u;
    e.n_rp = e.b.L * (e.b.L - 1u) / 2u;
    e.ranged = !mcq_ext_opp_all(er);
    for (uint32_t i = 0; i < 6; i++) e.bits[i] = er.w[er.opp_set() + i];
    return MCQ_XX_OK;
}

// range bits of the hand at R-positions pa < pb (r_id[p] = card id of R-position p): bit 0 cls(pa, pb), bit j (j = 1..3)
// cls(pa, pb - j) when pb - j > pa -- what the weights of mcq_exact_ext_w1 / _w2 test
MCQ_HD uint32_t mcq_exact_ext_cbits(const McqExactExtQuery &e, const uint8_t *r_id, uint32_t pa, uint32_t pb) {
    uint32_t c = mcq_in_range(e.bits, r_id[pa], r_id[pb]) ? 1u : 0u;
#pragma unroll
    for (uint32_t j = 1; j <= 3; j++)
        if (pb >= pa + j + 1u && mcq_in_range(e.bits, r_id[pa], r_id[pb - j])) c |= 1u << j;
    return c;
}

// weight of the first opponent's hand
MCQ_HD uint32_t mcq_exact_ext_w1(bool ref_law, uint32_t cb, uint32_t pa, uint32_t pb) {
    if (!ref_law) return cb & 1u;
    return (cb & 1u) + (pb != pa + 1u ? (cb >> 1) & 1u : 0u);
}

// weight of the second opponent's hand {pa < pb} once the first hand {qa < qb} has left the deck
MCQ_HD uint32_t mcq_exact_ext_w2(bool ref_law, uint32_t cb, uint32_t pa, uint32_t pb, uint32_t qa, uint32_t qb) {
    if (!ref_law) return cb & 1u;
    uint32_t prev = pb - 1u; /* the deck card below pb: skip the first hand (qb first: it lies above qa) */
    prev -= prev == qb ? 1u : 0u;
    prev -= prev == qa ? 1u : 0u;
    return (cb & 1u) + (prev != pa ? (cb >> (pb - prev)) & 1u : 0u);
}

// packed record of a candidate hand for one completion: R-positions, how many lie above the highest new table card,
// range bits
MCQ_HD uint32_t mcq_exact_ext_pack(uint32_t pa, uint32_t pb, uint32_t top, bool any_new, uint32_t cb) {
    const uint32_t above = any_new ? (pa > top ? 1u : 0u) + (pb > top ? 1u : 0u) : 0u;
    return pa | (pb << 6) | (above << 12) | (cb << 14);
}
MCQ_HD uint32_t mcq_exact_ext_cb(uint32_t r) { return r >> 14; }
MCQ_HD uint32_t mcq_exact_ext_above(uint32_t r) { return (r >> 12) & 3u; }

// The known hands of one completion in ONE pass (wave-uniform); a caller that ignores a part leaves it to the compiler to
// drop after inlining.
//   best   the strongest known hand's key, 0 without known hands (every hand's key is > 0);
//   n_eq   the known hands whose key equals hero's (split-pot form: the pot of a tie is shared by 1 + n_eq hands, by
//          2 + n_eq when the one candidate hand is level with hero too);
//   top    the greatest key among hero (seat 0) and the known hands (seats 1..n_known), level = the mask of the seats
//          that hold it (per-seat form).
struct McqExactKnown {
    uint32_t best, n_eq, top, level;
};
MCQ_HD McqExactKnown mcq_exact_ext_known(const McqExactExtQuery &e, const McqExactBoard &bd, const uint32_t *tf,
                                         const uint32_t *tops, const uint32_t *sd) {
    McqExactKnown kn = {0u, 0u, bd.hero_key, 1u};
    for (uint32_t h = 0; h < e.n_known; h++) {
        McqHole kh;
        kh.set(mcq_card(e.known[h] & 0xFFu), mcq_card(e.known[h] >> 8));
        const uint32_t key = mcq_eval_key(bd.b, bd.fs, kh, tf, tops, sd);
        kn.best = key > kn.best ? key : kn.best;
        kn.n_eq += key == bd.hero_key ? 1u : 0u;
        kn.level = key > kn.top ? 0u : kn.level;
        kn.level |= key >= kn.top ? 2u << h : 0u;
        kn.top = key > kn.top ? key : kn.top;
    }
    return kn;
}

// Split-pot form (kinds 0 and 1: at most one random opponent).  The tie weights are split by k = the hands that share
// the pot, hero included.  Per completion the known hands' count n_eq is wave-uniform, so a lane keeps ONE further sum --
// tie_c, the ties in which the candidate's key equals hero's: those are shared by 2 + n_eq hands, the other ties
// (tie - tie_c: the candidate below hero, a known hand level) by 1 + n_eq.
struct McqExactAccWays {
    static constexpr bool kWays = true;
    uint32_t win, tie, tot;
    uint32_t tie_c; /* part of `tie` in which the candidate hand's own key equals hero's */
};

struct McqExactExtSums { /* 64-bit: a first hand's sums over all completions */
    unsigned long long win, tie, tot, type[9];
};

// Word `word` of one completion's row from its sums over the candidate hands: runs, passes = 0, win, tie, by_type[9] --
// hero's hand type is fixed per completion: one entry, win + tie --, then tie_ways[9] (22-word rows of mcq_result_ways
// only; a plain row ends at word 13 and passes tie_c = n_eq = 0).  Those ties are shared by 2 + n_eq hands where the
// candidate is level with hero (tie_c), the others by 1 + n_eq (n_eq >= 1 there).  No random opponent: tie_c = 0.
MCQ_HD unsigned long long mcq_exact_ext_row_word(uint32_t word, uint32_t win, uint32_t tie, uint32_t tot, uint32_t tie_c,
                                                 uint32_t type, uint32_t n_eq) {
    if (word < 4u) return word == 0u ? tot : word == 2u ? win : word == 3u ? tie : 0u;
    if (word < 13u) return word - 4u == type ? win + tie : 0u;
    const uint32_t j = word - 13u;
    return (j == n_eq ? tie_c : 0u) + (j + 1u == n_eq ? tie - tie_c : 0u);
}

// No random opponent: completion `idx` alone (one lane) -- its R-positions, board and known hands; returns its weight
// (0 or 1).  The plain, split-pot, per-seat and per-runout forms all start here.
MCQ_HD uint32_t mcq_exact_ext_lone_known(const McqExactExtQuery &e, uint32_t idx, const uint32_t *sel8, const uint32_t *tf,
                                   const uint32_t *tops, const uint32_t *sd, uint32_t pos[5], McqExactBoard &bd,
                                   McqExactKnown &kn) {
    mcq_exact_unrank(idx, e.b.L, e.b.k, pos);
    mcq_exact_board(e.b, pos, sel8, tf, tops, sd, bd);
    kn = mcq_exact_ext_known(e, bd, tf, tops, sd);
    return !e.b.ref_law || bd.u > 0u ? 1u : 0u;
}
// ... and what it gives hero: a win above every known hand, a tie level with the best of them (shared by 1 + kn.n_eq hands)
MCQ_HD McqExactAcc mcq_exact_ext_lone_acc(const McqExactBoard &bd, const McqExactKnown &kn, uint32_t w) {
    return {kn.best < bd.hero_key ? w : 0u, kn.best == bd.hero_key ? w : 0u, w};
}

// the range bits of every R-pair (index pb (pb - 1) / 2 + pa): they do not depend on the completion; entries rp, rp + step, ...
MCQ_HD void mcq_exact_ext_cb_table(const McqExactExtQuery &e, const uint8_t *r_id, uint32_t rp0, uint32_t step, uint8_t *cb_tab) {
    for (uint32_t rp = rp0; rp < e.n_rp; rp += step) {
        uint32_t pa, pb;
        mcq_exact_pair_xy(rp, pa, pb);
        cb_tab[rp] = (uint8_t)mcq_exact_ext_cbits(e, r_id, pa, pb);
    }
}

// The candidate hands lane, lane + n_lanes, ... of one completion (rem_card / rem_pos: the m cards left, pair_xy as in
// mcq_exact.hpp; cb_tab from mcq_exact_ext_cb_table): on(i, pa, pb, key, r, w) gets candidate i's R-positions, its own key,
// its packed record and its weight as the FIRST opponent's hand (0 where the reference law's completion condition fails).
// The three bodies below say only what they do with a candidate.
template <class On>
MCQ_HD void mcq_exact_ext_candidates(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t lane, uint32_t n_lanes,
                                     const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos,
                                     const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, On on) {
    for (uint32_t i = lane; i < e.n_pairs; i += n_lanes) {
        const uint32_t xy = pair_xy[i], x = xy & 0xFFu, y = xy >> 8;
        McqHole h;
        h.set(rem_card[x], rem_card[y]);
        const uint32_t key = mcq_eval_key(bd.b, bd.fs, h, tf, tops, sd);
        const uint32_t pa = rem_pos[x], pb = rem_pos[y];
        const uint32_t r = mcq_exact_ext_pack(pa, pb, bd.top, e.b.k != 0u, cb_tab[pb * (pb - 1u) / 2u + pa]);
        const bool ok = !e.b.ref_law || mcq_exact_ext_above(r) < bd.u;
        on(i, pa, pb, key, r, ok ? mcq_exact_ext_w1(e.b.ref_law, mcq_exact_ext_cb(r), pa, pb) : 0u);
    }
}

// Pass A, one opponent: the outcome of every candidate, its key raised to the known hands' best kb, is tallied.
// Acc = McqExactAccWays: tie_c is kept beside the tallies.
template <class Acc>
MCQ_HD void mcq_exact_ext_pass_a_tally(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t kb, uint32_t lane,
                                 uint32_t n_lanes, const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos,
                                 const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, Acc &acc) {
    mcq_exact_ext_candidates(e, bd, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd,
                             [&](uint32_t, uint32_t, uint32_t, uint32_t own, uint32_t, uint32_t w) {
                                 const uint32_t key = own > kb ? own : kb;
                                 acc.win += key < bd.hero_key ? w : 0u;
                                 acc.tie += key == bd.hero_key ? w : 0u;
                                 acc.tot += w;
                                 if constexpr (Acc::kWays) acc.tie_c += own == bd.hero_key && key == bd.hero_key ? w : 0u;
                             });
}
// Pass A, two opponents: the raised key and the packed record are stored for pass B.
MCQ_HD void mcq_exact_ext_pass_a_store(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t kb, uint32_t lane,
                                       uint32_t n_lanes, const uint16_t *pair_xy, const McqCard *rem_card,
                                       const uint32_t *rem_pos, const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops,
                                       const uint32_t *sd, uint32_t *keys, uint32_t *rec) {
    mcq_exact_ext_candidates(e, bd, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd,
                             [&](uint32_t i, uint32_t, uint32_t, uint32_t own, uint32_t r, uint32_t) {
                                 keys[i] = own > kb ? own : kb;
                                 rec[i] = r;
                             });
}

// Per SEAT with ONE random opponent (mcq_exact_ext_kernel<1, MCQ_ROW_SEATS>).  Per completion the best key among hero and
// the known hands, the mask `level` of the seats holding it and their number n are wave-uniform (McqExactKnown: top,
// level), and a candidate hand is above, level with or below that key: a lane keeps THREE sums, the weight above (gt),
// level (eq) and in all (tot); the weight below is tot - gt - eq.
struct McqExactAccSeats {
    uint32_t gt, eq, tot;
};
MCQ_HD void mcq_exact_ext_pass_seats(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t best, uint32_t lane,
                                     uint32_t n_lanes, const uint16_t *pair_xy, const McqCard *rem_card,
                                     const uint32_t *rem_pos, const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops,
                                     const uint32_t *sd, McqExactAccSeats &acc) {
    mcq_exact_ext_candidates(e, bd, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd,
                             [&](uint32_t, uint32_t, uint32_t, uint32_t key, uint32_t, uint32_t w) {
                                 acc.gt += key > best ? w : 0u;
                                 acc.eq += key == best ? w : 0u;
                                 acc.tot += w;
                             });
}
// What one completion adds to word `word` of the mcq_result_seats row, from its three sums over all candidates: word 0 is
// runs, word 2 + 3 s + f is win / tie / share (f = 0, 1, 2) of seat s; the random opponent sits at seat 1 + n_known.
//   random opponent: wins gt, ties eq, share 2520 gt + 2520 / (n + 1) eq
//   a level seat:    wins lt if it is alone (n == 1), else ties lt; ties eq; share 2520 / n lt + 2520 / (n + 1) eq
// One random opponent leaves at most eight known hands: n + 1 <= 10, the shares come from mcq_seat_increment's table.
// tot <= 2 x 990 per completion: the products fit 32 bits; the caller's running sums are 64-bit.
MCQ_HD uint32_t mcq_exact_ext_seats_word(uint32_t word, uint32_t level, uint32_t n_known, uint32_t gt, uint32_t eq,
                                         uint32_t tot) {
    if (word < 2u) return word == 0u ? tot : 0u;
    const uint32_t s = (word - 2u) / 3u, f = (word - 2u) - 3u * s;
    const uint32_t n = mcq_popc(level), lt = tot - gt - eq;
    const uint32_t with_opp = mcq_seat_increment(n + 1u) & 0xFFFFu;
    if (s == 1u + n_known) return f == 0u ? gt : f == 1u ? eq : MCQ_SHARE_UNIT * gt + with_opp * eq;
    if (((level >> s) & 1u) == 0u) return 0u;
    const uint32_t alone = mcq_seat_increment(n) & 0xFFFFu;
    return f == 0u ? (n == 1u ? lt : 0u) : f == 1u ? eq + (n > 1u ? lt : 0u) : alone * lt + with_opp * eq;
}

// Pass B for ONE first hand h1 = R-positions qa < qb: its M-index in this completion, or n_pairs when a new table card
// took one of its cards
MCQ_HD uint32_t mcq_exact_ext_m_index(const McqExactExtQuery &e, const uint32_t pos[5], uint32_t qa, uint32_t qb) {
    uint32_t xa = qa, xb = qb;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++) {
        if (pos[i] == qa || pos[i] == qb) return e.n_pairs; /* unused entries are 255 */
        xa -= pos[i] < qa ? 1u : 0u;
        xb -= pos[i] < qb ? 1u : 0u;
    }
    return xb * (xb - 1u) / 2u + xa;
}

// ... and every second hand of the completion against it (keys / rec from pass A): the weights w2 of the outcomes
MCQ_HD void mcq_exact_ext_pass_b(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t qa, uint32_t qb, uint32_t mi,
                                 const uint32_t *keys, const uint32_t *rec, McqExactAcc &acc) {
    const uint32_t k1 = keys[mi], a1 = mcq_exact_ext_above(rec[mi]);
    const bool ref = e.b.ref_law;
    for (uint32_t p2 = 0; p2 < e.n_pairs; p2++) {
        const uint32_t r2 = rec[p2], pa = r2 & 63u, pb = (r2 >> 6) & 63u;
        const bool shared = pa == qa || pa == qb || pb == qa || pb == qb;
        const bool ok = !shared && (!ref || a1 + mcq_exact_ext_above(r2) < bd.u);
        const uint32_t w = ok ? mcq_exact_ext_w2(ref, mcq_exact_ext_cb(r2), pa, pb, qa, qb) : 0u;
        const uint32_t k2 = keys[p2], km = k1 > k2 ? k1 : k2;
        acc.win += km < bd.hero_key ? w : 0u;
        acc.tie += km == bd.hero_key ? w : 0u;
        acc.tot += w;
    }
}

MCQ_HD void mcq_exact_ext_add(McqExactExtSums &s, const McqExactAcc &a, uint32_t type) {
    s.win += a.win;
    s.tie += a.tie;
    s.tot += a.tot;
#pragma unroll
    for (uint32_t t = 0; t < 9; t++) s.type[t] += t == type ? (unsigned long long)(a.win + a.tie) : 0ull;
}

// R's card ids by position
MCQ_HD void mcq_exact_ext_r_ids(const McqExactExtQuery &e, uint8_t *r_id) {
    uint32_t lo = e.b.deck_lo, hi = e.b.deck_hi, n = 0;
    for (uint32_t c = 0; c < 52; c++)
        if (((c < 32 ? lo >> c : hi >> (c - 32u)) & 1u) != 0u) r_id[n++] = (uint8_t)c;
}

// ---- host side: what the enumeration needs up front and how its sums become the result
// Can every random opponent be dealt on every branch that has positive probability?  (The reference would loop forever.)
MCQ_HD bool mcq_exact_ext_dealable(const McqExactExtQuery &e, const uint8_t *r_id) {
    if (e.b.n_opp == 0u) return true;
    bool any = false;
    for (uint32_t qb = 1; qb < e.b.L; qb++)
        for (uint32_t qa = 0; qa < qb; qa++) {
            if (!mcq_exact_ext_w1(e.b.ref_law, mcq_exact_ext_cbits(e, r_id, qa, qb), qa, qb)) continue;
            any = true;
            if (e.b.n_opp < 2u) return true;
            bool second = false;
            for (uint32_t pb = 1; pb < e.b.L && !second; pb++)
                for (uint32_t pa = 0; pa < pb && !second; pa++)
                    if (pa != qa && pa != qb && pb != qa && pb != qb)
                        second = mcq_exact_ext_w2(e.b.ref_law, mcq_exact_ext_cbits(e, r_id, pa, pb), pa, pb, qa, qb) != 0u;
            if (!second) return false;
        }
    return any;
}

// Are the outcomes' probabilities integer weights over one common total?  (Not with two ranged opponents.)
MCQ_HD bool mcq_exact_ext_has_weights(const McqExactExtQuery &e) { return e.b.n_opp < 2u || !e.ranged; }

// The result of one query.  w: in, the tallies of the enumeration when there are fewer than two random opponents; out, the
// integer weights (zeroed without them).  h1: the per-first-hand sums of a two-opponent enumeration (n_rp x MCQ_XX_SUMS),
// combined in first-hand order.
MCQ_HD void mcq_exact_ext_finish(const McqExactExtQuery &e, const uint8_t *r_id, const unsigned long long *h1, mcq_result &w,
                                 mcq_exact_prob &p) {
    if (e.b.n_opp == 2u) {
        double num[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, n1 = 0;
        uint64_t sum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t rp = 0; rp < e.n_rp; rp++) {
            uint32_t qa, qb;
            mcq_exact_pair_xy(rp, qa, qb);
            const uint32_t w1 = mcq_exact_ext_w1(e.b.ref_law, mcq_exact_ext_cbits(e, r_id, qa, qb), qa, qb);
            const unsigned long long *s = h1 + (size_t)rp * MCQ_XX_SUMS;
            if (w1 == 0u || s[2] == 0ull) continue;
            for (uint32_t j = 0; j < 12; j++) sum[j] += (uint64_t)w1 * s[j];
            n1 += (double)w1;
            const double f = (double)w1 / (double)s[2];
            num[0] += f * (double)s[0];
            num[1] += f * (double)s[1];
            for (uint32_t t = 0; t < 9; t++) num[2 + t] += f * (double)s[3 + t];
        }
        w.passes = 0;
        w.runs = sum[2];
        w.win = sum[0];
        w.tie = sum[1];
        for (uint32_t t = 0; t < 9; t++) w.by_type[t] = sum[3 + t];
        if (e.ranged) {
            p.win = num[0] / n1;
            p.tie = num[1] / n1;
            for (uint32_t t = 0; t < 9; t++) p.by_type[t] = num[2 + t] / n1;
            w = mcq_result{};
            return;
        }
    }
    const double runs = (double)w.runs;
    p.win = (double)w.win / runs;
    p.tie = (double)w.tie / runs;
    for (uint32_t t = 0; t < 9; t++) p.by_type[t] = (double)w.by_type[t] / runs;
}

// ---- the pieces above BY THE NAMES and with the argument lists that the host simulators of the tests call (one-line
// instances, as in mcq_exact_hero.hpp: the simulators' sources stay what they were, so the host tests pin the shared code
// as they pinned the copies).  The kernels call the pieces themselves.
MCQ_HD uint32_t mcq_exact_ext_known_best(const McqExactExtQuery &e, const McqExactBoard &bd, const uint32_t *tf,
                                         const uint32_t *tops, const uint32_t *sd) {
    return mcq_exact_ext_known(e, bd, tf, tops, sd).best;
}
MCQ_HD uint32_t mcq_exact_ext_known_best_eq(const McqExactExtQuery &e, const McqExactBoard &bd, const uint32_t *tf,
                                            const uint32_t *tops, const uint32_t *sd, uint32_t &n_eq) {
    const McqExactKnown kn = mcq_exact_ext_known(e, bd, tf, tops, sd);
    n_eq = kn.n_eq;
    return kn.best;
}
MCQ_HD uint32_t mcq_exact_ext_level_seats(const McqExactExtQuery &e, const McqExactBoard &bd, const uint32_t *tf,
                                          const uint32_t *tops, const uint32_t *sd, uint32_t &level) {
    const McqExactKnown kn = mcq_exact_ext_known(e, bd, tf, tops, sd);
    level = kn.level;
    return kn.top;
}
// completion `idx` alone: its tallies added to acc, -> hero's hand type; n_eq as above
MCQ_HD uint32_t mcq_exact_ext_lone_ways(const McqExactExtQuery &e, uint32_t idx, const uint32_t *sel8, const uint32_t *tf,
                                        const uint32_t *tops, const uint32_t *sd, McqExactAcc &acc, uint32_t &n_eq) {
    uint32_t pos[5];
    McqExactBoard bd;
    McqExactKnown kn;
    const uint32_t w = mcq_exact_ext_lone_known(e, idx, sel8, tf, tops, sd, pos, bd, kn);
    const McqExactAcc a = mcq_exact_ext_lone_acc(bd, kn, w);
    acc.win += a.win;
    acc.tie += a.tie;
    acc.tot += a.tot;
    n_eq = kn.n_eq;
    return mcq_key_type(bd.hero_key);
}
MCQ_HD uint32_t mcq_exact_ext_lone(const McqExactExtQuery &e, uint32_t idx, const uint32_t *sel8, const uint32_t *tf,
                                   const uint32_t *tops, const uint32_t *sd, McqExactAcc &acc) {
    uint32_t n_eq;
    return mcq_exact_ext_lone_ways(e, idx, sel8, tf, tops, sd, acc, n_eq);
}
// ... per seat: -> its weight, the level seats' mask and their number k
MCQ_HD uint32_t mcq_exact_ext_lone_seats(const McqExactExtQuery &e, uint32_t idx, const uint32_t *sel8, const uint32_t *tf,
                                         const uint32_t *tops, const uint32_t *sd, uint32_t &level, uint32_t &k) {
    uint32_t pos[5];
    McqExactBoard bd;
    McqExactKnown kn;
    const uint32_t w = mcq_exact_ext_lone_known(e, idx, sel8, tf, tops, sd, pos, bd, kn);
    level = kn.level;
    k = mcq_popc(level);
    return w;
}
// pass A with both forms behind one argument list: keys == nullptr tallies, else key and record are stored
template <class Acc>
MCQ_HD void mcq_exact_ext_pass_a(const McqExactExtQuery &e, const McqExactBoard &bd, uint32_t kb, uint32_t lane,
                                 uint32_t n_lanes, const uint16_t *pair_xy, const McqCard *rem_card, const uint32_t *rem_pos,
                                 const uint8_t *cb_tab, const uint32_t *tf, const uint32_t *tops, const uint32_t *sd,
                                 uint32_t *keys, uint32_t *rec, Acc &acc) {
    if (keys) mcq_exact_ext_pass_a_store(e, bd, kb, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd, keys, rec);
    else mcq_exact_ext_pass_a_tally(e, bd, kb, lane, n_lanes, pair_xy, rem_card, rem_pos, cb_tab, tf, tops, sd, acc);
}

#endif /* MCQ_EXACT_EXT_HPP */
