// mcq_ranges.hpp -- Monte-Carlo multiway equity with a WEIGHTED RANGE PER SEAT (mcq_eval_batch_ranges, include/mcq.h).
// Lane code and the record helpers, written MCQ_HD: mcq_kernels.hip compiles them for gfx950, mcq_host.cpp and
// tests/hostsim_ranges for the host.
//
// The law ("MCQ-RG v1").  A record is an mcq_query (hole ignored, 0/3/4/5 table cards B, p = n_players seats, 2..10) and
// one weight table w_s[1326] per seat (uint16, indexed by MCQ_HAND_INDEX).  eff_s(h) = w_s[h] if h holds no card of B,
// else 0.  One iteration deals
//     P(h_0, .., h_{p-1})  ~  prod_s eff_s(h_s) * [the hands are pairwise disjoint]
// and then the 5 - |B| missing table cards uniformly without replacement from the 52 - |B| - 2p cards left.  That is
// the JOINT law, symmetric in the seats -- not the sequential "first seat, then each further seat from what is left".
// It is realised by rejection, which is exact:
//   1. seat s draws a hand with probability w_s[h] / sum(w_s): ONE random word u per draw, t = mulhi32(u, total_s), the
//      hand is the first index in ascending MCQ_HAND_INDEX order whose inclusive cumulative weight exceeds t (the
//      probability of a hand is off by less than 2^-32: floor arithmetic on a 32-bit word);
//   2. that seat alone draws again while its hand holds a table card (the table is fixed: conditioning per seat);
//   3. when the hand shares a card with the hand of an earlier seat the WHOLE trial is abandoned -- at that seat, the
//      seats behind it do not draw -- and every seat draws again.
// `passes` counts the whole trials, accepted one included.  The table cards then come two per word with bound L = the
// cards left (every card: the reference law's "never the highest card" does not apply here).
// Words are taken from the stream of the extended path (McqExtCtrDraws, keyed by (seed, query id, task * 64 + lane),
// sixteen iterations per stream) in exactly this order, so a row depends on (record, tables, seed, query id) only.
//
// A prepared table is MCQ_RG_CUM_STRIDE uint32 words: the 1326 inclusive prefix sums (total <= 1326 * 65535 < 2^27), the
// last one being the total, then the number of non-zero entries and the index of the last of them.  It depends on the
// table alone -- the table cards are the per-seat re-draw's business -- so it is prepared once per DISTINCT table, not per
// record and seat.  A table with ONE non-zero entry is a KNOWN HAND: its seat holds that hand in every trial, draws no
// word and reads no table (the mapping would select that hand for every word), so the table per record that "hero holds
// these two cards" costs takes no room among the tables a block stages.
#pragma once
#include "mcq_device.hpp"

#define MCQ_RG_CUM_STRIDE 1328u   /* words per prepared table (16-byte multiple) */
#define MCQ_RG_TOTAL_WORD 1325u   /* the inclusive sum behind the last hand = the table's total */
#define MCQ_RG_NNZ_WORD 1326u     /* how many entries are not zero */
#define MCQ_RG_LAST_WORD 1327u    /* the index of the last of them */
#define MCQ_RG_KNOWN 0x80000000u  /* McqRangesWaveCtx::total of a known hand: this flag | a | b << 8 */
#define MCQ_RG_STAGE_TABLES 6u    /* prepared tables a block keeps in LDS beside the evaluator's (6 x 5312 B) */
#define MCQ_RG_HANDS_STAGE_TABLES 3u /* ... the per-hand kernel: 21 KB of its LDS hold the table of hands (mcq_hands.hpp) */
#define MCQ_RG_STAGE_QUERIES 32u /* a block looks at no more records than this when it decides what to stage */

/* the record: a valid table, 0/3/4/5 of its cards, 2..10 seats, at least one iteration; hole is not read */
MCQ_HD bool mcq_ranges_query_valid(const McqQueryWords &q) {
    const uint32_t nb = q.n_board();
    if (!(nb == 0u || (nb >= 3u && nb <= 5u)) || q.n_players() < 2u || q.n_players() > 10u || q.reserved() != 0u || q.runs() == 0u)
        return false;
    uint64_t seen = 0;
    bool ok = true;
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t c = q.card(2u + i);
        ok = ok && c < 52u && !((seen >> (c & 63u)) & 1u);
        seen |= 1ull << (c & 63u);
    }
    return ok;
}
MCQ_HD uint64_t mcq_ranges_board_mask(const McqQueryWords &q) {
    uint64_t m = 0;
    for (uint32_t i = 0; i < q.n_board(); i++) m |= 1ull << (q.card(2u + i) & 63u);
    return m;
}
/* wave tasks of a record (64 streams of MCQ_STREAM_ITERS iterations) and the price of one on the cost axis the kernel
 * cuts: the extended path's price for the same table and seats, which the kernels multiply by the host's ESTIMATE of the
 * record's whole trials per iteration (1 .. MCQ_RG_MAX_PRICE; from the seats' per-card weights, pair by pair, as if the
 * pairs of seats collided independently: scheduling only, a poor estimate costs balance, never a result). */
#define MCQ_RG_MAX_PRICE 256u
MCQ_HD uint32_t mcq_ranges_task_count(const McqQueryWords &q) { return mcq_task_count(q); }
MCQ_HD uint32_t mcq_ranges_task_weight(const McqQueryWords &q) { return 3u * mcq_task_weight(q) * (MCQ_STREAM_ITERS >> 1); }

MCQ_HD void mcq_ranges_hand(uint32_t idx, uint32_t &a, uint32_t &b);
/* host form of the preparation (the kernel scans in parallel; integer sums, the same words) */
MCQ_HD void mcq_ranges_prefix(const uint16_t *w, uint32_t *cum) {
    uint32_t at = 0, nnz = 0, last = 0;
    for (uint32_t i = 0; i < MCQ_HAND_ROWS; i++) {
        at += (uint32_t)w[i];
        cum[i] = at;
        nnz += w[i] != 0 ? 1u : 0u;
        last = w[i] != 0 ? i : last;
    }
    cum[MCQ_RG_NNZ_WORD] = nnz;
    cum[MCQ_RG_LAST_WORD] = last;
}
/* what the seat's entry of McqRangesWaveCtx::total is, from its prepared table */
MCQ_HD uint32_t mcq_ranges_seat_total(const uint32_t *cum) {
    if (cum[MCQ_RG_NNZ_WORD] != 1u) return cum[MCQ_RG_TOTAL_WORD];
    uint32_t a, b;
    mcq_ranges_hand(cum[MCQ_RG_LAST_WORD], a, b);
    return MCQ_RG_KNOWN | a | (b << 8);
}

/* MCQ_HAND_INDEX backwards: idx = b (b - 1) / 2 + a, a < b.  The square root is an estimate only (8 idx + 1 <= 10601 is
 * exact in a float; whatever the rounding of the root, the result is within one of b), the two integer steps make it
 * exact -- on the host and on the device alike. */
MCQ_HD void mcq_ranges_hand(uint32_t idx, uint32_t &a, uint32_t &b) {
    uint32_t e = (uint32_t)((1.0f + __builtin_sqrtf((float)(8u * idx + 1u))) * 0.5f);
    e = e * (e - 1u) / 2u > idx ? e - 1u : e;
    e = (e + 1u) * e / 2u <= idx ? e + 1u : e;
    b = e;
    a = idx - e * (e - 1u) / 2u;
}

struct McqRangesCtx { /* wave-uniform */
    uint32_t base_lo, base_hi; /* the 52 cards minus the table's */
    uint32_t n_players, n_deal, runs, L; /* L = cards left when the table is dealt: 52 - n_board - 2 n_players */
    McqBoard board;
};
struct McqRangesWaveCtx { /* per wave, in LDS: what the iteration indexes by seat at run time */
    uint32_t total[MCQ_MAX_SEATS];       /* the seat's table total (> 0, < 2^27), or MCQ_RG_KNOWN | its one hand */
    const uint32_t *cum[MCQ_MAX_SEATS];  /* its prepared table: HBM, or the block's LDS when the block has staged it */
};
MCQ_HD void mcq_ranges_ctx(const McqQueryWords &q, McqRangesCtx &c) {
    const uint64_t base = ((1ull << 52) - 1ull) & ~mcq_ranges_board_mask(q);
    c.board.clear();
    for (uint32_t i = 0; i < q.n_board(); i++) c.board.add(mcq_card(q.card(2u + i)));
    c.base_lo = (uint32_t)base;
    c.base_hi = (uint32_t)(base >> 32);
    c.n_players = q.n_players();
    c.n_deal = 5u - q.n_board();
    c.runs = q.runs();
    c.L = 52u - q.n_board() - 2u * q.n_players();
}

#if !defined(__HIP_DEVICE_COMPILE__) && defined(MCQ_RANGES_DEAL_HOOK)
#define MCQ_RG_DEALT(h, c1, c2) MCQ_RANGES_DEAL_HOOK(h, c1, c2) /* host test builds only: the hands of the iteration */
#else
#define MCQ_RG_DEALT(h, c1, c2) ((void)0)
#endif

// One iteration.  ids: this lane's slot array (stride `ids_stride`) for the seats' hands -- all of them travel through
// it as card ids, as in mcq_iteration_ext: ten hands do not fit the registers beside the evaluator, and the trial loop
// rewrites them at every abandoned trial anyway.  The deck is one 64-bit mask per lane.  LDS_TAB: the caller knows that
// every wc.cum[] of the record lies in LDS, so a draw's eleven dependent loads (word -> t -> binary search) use 32-bit
// LDS addresses instead of generic pointers (a flat load waits for both memory counters).
// Returns false when no trial was accepted within MCQ_EXT_MAX_TRIALS (seats that block each other) or a seat found no
// hand clear of the table within as many re-draws.
template <class Draws, bool LDS_TAB, class Acc>
MCQ_HD bool mcq_iteration_ranges(const McqRangesCtx &qc, const McqRangesWaveCtx &wc, Draws &dr, const McqCard *cards,
                                 const uint32_t *sel8, uint16_t *ids, uint32_t ids_stride, const uint32_t *tf,
                                 const uint32_t *tops, const uint32_t *sd, Acc &acc) {
    static_assert(Acc::kSeats, "the ranges entry writes per-seat rows");
    const uint64_t base = ((uint64_t)qc.base_hi << 32) | qc.base_lo;
    uint64_t deck = base;
    bool ok = false, dealable = true;
    uint32_t trial = 0;
    for (; trial < MCQ_EXT_MAX_TRIALS && !ok && dealable; trial++) {
        deck = base;
        ok = true;
        for (uint32_t s = 0; s < qc.n_players && ok; s++) {
            const uint32_t total = wc.total[s];
            const uint32_t *cum_g = wc.cum[s];
#if defined(__HIP_DEVICE_COMPILE__)
            typedef __attribute__((address_space(3))) const uint32_t *LdsCum;
            const LdsCum cum_l = (LdsCum)(uintptr_t)cum_g; /* (the low half of a generic LDS address is the LDS address) */
#define MCQ_RG_CUM(i) (LDS_TAB ? cum_l[i] : cum_g[i])
#else
#define MCQ_RG_CUM(i) (cum_g[i])
#endif
            uint32_t a = total & 0xFFu, b = (total >> 8) & 0xFFu; /* (a known hand; the host has seen it clear of the table) */
            bool clear = (total & MCQ_RG_KNOWN) != 0u && (((base >> a) & (base >> b)) & 1u) != 0u;
            const uint32_t budget = (total & MCQ_RG_KNOWN) ? 0u : MCQ_EXT_MAX_TRIALS; /* (wave-uniform) */
            for (uint32_t redraw = 0; redraw < budget && !clear; redraw++) {
                const uint32_t t = dr.pick(total);
                uint32_t pos = 0; /* hands whose inclusive sum is <= t = the first index whose sum exceeds t */
#pragma unroll
                for (uint32_t step = 1024u; step != 0u; step >>= 1) {
                    const uint32_t np = pos + step; /* (np - 1 clamped: the read stays inside the table) */
                    const uint32_t v = MCQ_RG_CUM(np - 1u < MCQ_RG_TOTAL_WORD ? np - 1u : MCQ_RG_TOTAL_WORD);
                    pos = np <= MCQ_HAND_ROWS && v <= t ? np : pos;
                }
                pos = pos < MCQ_HAND_ROWS ? pos : MCQ_HAND_ROWS - 1u; /* (t < total: never taken) */
                mcq_ranges_hand(pos, a, b);
                clear = (((base >> a) & (base >> b)) & 1u) != 0u;
            }
#undef MCQ_RG_CUM
            dealable = dealable && clear;
            ok = clear && (((deck >> a) & (deck >> b)) & 1u) != 0u;
            deck &= ~(((uint64_t)1 << a) | ((uint64_t)1 << b));
            ids[s * ids_stride] = (uint16_t)(a | (b << 8));
        }
    }
    acc.passes += trial;
    if (!ok) return false;
    uint32_t dlo = (uint32_t)deck, dhi = (uint32_t)(deck >> 32);
    uint32_t L = qc.L; /* wave-uniform: every lane has dealt two cards per seat */
    McqBoard b = qc.board;
    for (uint32_t k = 0; k < qc.n_deal; k++, L--) {
        const uint32_t c = mcq_select_pop(dlo, dhi, dr.table(k, L), sel8);
        MCQ_RG_DEALT(0x100u + k, c, 0u);
        b.add(cards[c < 52u ? c : 0u]);
    }
    McqFlushSel fs;
    fs.from_board(b);
    uint32_t best = 0, level = 0; /* the best key of ALL hands and the seats that hold it */
    for (uint32_t h = 0; h < qc.n_players; h++) {
        const uint32_t v = ids[h * ids_stride];
        MCQ_RG_DEALT(h, v & 0xFFu, (v >> 8) & 0xFFu);
        McqHole hh;
        hh.set(cards[v & 0xFFu], cards[(v >> 8) & 0xFFu]);
        const uint32_t k = mcq_eval_key(b, fs, hh, tf, tops, sd);
        level = k > best ? 0u : level;
        level |= k >= best ? 1u << h : 0u;
        best = k > best ? k : best;
    }
    const uint32_t inc = mcq_seat_increment(mcq_popc(level));
#pragma unroll
    for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) acc.seat[s] += ((level >> s) & 1u) ? inc : 0u;
    acc.dealt(ids, ids_stride, level, inc); /* (McqLaneAccSeats: empty; mcq_hands.hpp: the watched seat's hand) */
    return true;
}
