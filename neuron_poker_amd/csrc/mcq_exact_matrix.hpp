// mcq_exact_matrix.hpp -- the exact hand-against-hand matrix of a board (mcq_exact_matrix, include/mcq.h): every two-card
// hand against every other one, heads-up, uniform law, from ONE enumeration; lane code shared by the three
// mcq_exact_matrix_*_kernel (mcq_kernels.hip) and the host build of the tests (tests/hostsim_matrix).  The pieces of
// mcq_exact.hpp and mcq_exact_hero.hpp are reused unchanged.
//
// What is enumerated.  D = 52 cards minus table and dead cards, ascending card id; L = |D| <= 49.  Positions run over D; a
// D-pair is a hand at D-positions qa < qb with index qb (qb - 1) / 2 + qa, n_rp = C(L, 2) <= 1176 of them.  The completions
// are the k-subsets T of D (k = 5 - n_board <= 2), n_boards = C(L, k) <= 1176.  For two disjoint hands h, g the completions
// that miss both number total = C(L - 4, k) whatever the hands: win[h][g] counts those on which h ranks strictly above g.
// Three steps:
//   ranking   one word per (completion, D-pair): 0 when the pair holds a card of T (it is DEAD on T), else its key + 1
//             (mcq_matrix_rank; keys stay below 0xA0000000, so a live word lies strictly between 0 and 0xFFFFFFFF);
//   counting  a register tile of TH x TG counters advanced by one completion (mcq_matrix_count): TH row words as they are
//             and TG column words with the dead mark turned into 0xFFFFFFFF (mcq_matrix_col), so that [row > col] is false
//             whenever either hand is dead on T and the loop needs no liveness test.  Pairs of hands that share a card are
//             counted like any other and masked afterwards;
//   finish    entry (r, c) of the [1326][1326] matrices from the counts by D-pair (mcq_matrix_entry): win = the count,
//             tie = total - count[h][g] - count[g][h] for disjoint hands of D, 0 everywhere else.
// The words are kept as 32-bit keys, not compressed to 16-bit dense ranks per completion: that would take a sort (or a
// 1176-wide rank count) per completion in the ranking kernel to halve the bytes of a table that is read from L2 once per
// tile row, and the count loop compares 32-bit registers either way.
#ifndef MCQ_EXACT_MATRIX_HPP
#define MCQ_EXACT_MATRIX_HPP

#include "mcq_exact_hero.hpp"

#define MCQ_XM_TILE 64u    /* D-pairs per side of a count tile: one block */
#define MCQ_XM_TH 4u       /* a thread's counters: TH row hands ... */
#define MCQ_XM_TG 4u       /* ... by TG column hands */
#define MCQ_XM_STAGE 16u   /* completions per LDS stage of the count loop */
#define MCQ_XM_MAX_STRIDE ((MCQ_XH_MAX_HANDS + MCQ_XM_TILE - 1u) / MCQ_XM_TILE * MCQ_XM_TILE) /* 1216: D-pairs padded to whole tiles */
#define MCQ_XM_MAX_BOARDS ((MCQ_XH_MAX_HANDS + MCQ_XM_STAGE - 1u) / MCQ_XM_STAGE * MCQ_XM_STAGE) /* 1184: completions padded to whole stages */
#define MCQ_XM_NO_PAIR 0xFFFFu /* mcq_matrix_hands: a card of the hand is not in D */

static_assert(MCQ_MATRIX_MAX_BATCH == 256u && sizeof(mcq_matrix_query) == 16u, "include/mcq.h");
static_assert(45u * 44u / 2u == 990u && 990u <= 0xFFFFu, "total = C(L - 4, k) <= C(45, 2) = 990: the entries are uint16_t");
static_assert(MCQ_XH_MAX_HANDS < MCQ_XM_NO_PAIR, "a D-pair index is not the mark");
static_assert(MCQ_XH_ROWS == MCQ_HAND_ROWS, "the matrices are [MCQ_HAND_ROWS][MCQ_HAND_ROWS]");
static_assert(((uint32_t)MCQ_C_SF + 1u) << MCQ_KEY_SHIFT < 0xFFFFFFFFu - 1u, "key + 1 of a live hand stays below the column's dead mark");
static_assert(MCQ_XM_TILE % MCQ_XM_TH == 0u && MCQ_XM_TILE % MCQ_XM_TG == 0u, "whole register tiles");

/* why a record is refused (0 = it is not), tested in this order */
#define MCQ_XM_OK 0
#define MCQ_XM_STREET 1     /* n_board not in 3..5 */
#define MCQ_XM_RESERVED 2   /* reserved bytes not 0 */
#define MCQ_XM_MASK 3       /* bits 52..63 of the dead mask */
#define MCQ_XM_CARD 4       /* a table card id >= 52 */
#define MCQ_XM_TWICE 5      /* a table card twice */
#define MCQ_XM_DEAD_TABLE 6 /* a table card that is also dead */
#define MCQ_XM_SHORT 7      /* L - 4 < k */

struct McqMatrixQuery { /* block-uniform */
    McqExactQuery b;    /* deck = D, L, k, known = the table cards (no hero, uniform law) */
    uint32_t n_rp;      /* C(L, 2) D-pairs */
    uint32_t n_boards;  /* C(L, k) completions */
    uint32_t total;     /* C(L - 4, k) */
};

MCQ_HD int mcq_matrix_query_build(const mcq_matrix_query &q, McqMatrixQuery &e) {
    if (q.n_board < 3u || q.n_board > 5u) return MCQ_XM_STREET;
    if (q.reserved[0] != 0u || q.reserved[1] != 0u) return MCQ_XM_RESERVED;
    if ((q.dead >> 52) != 0u) return MCQ_XM_MASK;
    uint64_t table = 0;
    for (uint32_t i = 0; i < q.n_board; i++) {
        const uint32_t c = q.board[i];
        if (c >= 52u) return MCQ_XM_CARD;
        if ((table >> c) & 1u) return MCQ_XM_TWICE;
        table |= 1ull << c;
    }
    if ((table & q.dead) != 0u) return MCQ_XM_DEAD_TABLE;
    const uint64_t deck = ((1ull << 52) - 1ull) & ~(table | q.dead);
    e.b.deck_lo = (uint32_t)deck;
    e.b.deck_hi = (uint32_t)(deck >> 32);
    e.b.L = mcq_popc(e.b.deck_lo) + mcq_popc(e.b.deck_hi);
    e.b.k = 5u - q.n_board;
    if (e.b.L < e.b.k + 4u) return MCQ_XM_SHORT;
    e.b.n_opp = 1u;
    e.b.ref_law = false;
    e.b.known.clear();
    for (uint32_t i = 0; i < q.n_board; i++) e.b.known.add(mcq_card(q.board[i]));
    e.b.hero.set(mcq_card(0u), mcq_card(1u)); /* (nobody's) */
    e.n_rp = e.b.L * (e.b.L - 1u) / 2u;
    e.n_boards = mcq_exact_binom(e.b.L, e.b.k);
    e.total = mcq_exact_binom(e.b.L - 4u, e.b.k);
    return MCQ_XM_OK;
}

/* D-pairs padded to whole tiles: the row length of the key table and of the counts, and the rows of the counts */
MCQ_HD uint32_t mcq_matrix_stride(uint32_t n_rp) { return (n_rp + MCQ_XM_TILE - 1u) / MCQ_XM_TILE * MCQ_XM_TILE; }
/* completions padded to whole stages: the rows of the key table (the padding rows hold dead marks only) */
MCQ_HD uint32_t mcq_matrix_stages(uint32_t n_boards) { return (n_boards + MCQ_XM_STAGE - 1u) / MCQ_XM_STAGE; }

/* card ids of D by position (64 entries, zero at and above L) */
MCQ_HD void mcq_matrix_r_ids(const McqMatrixQuery &e, uint8_t *r_id) {
    uint32_t n = 0;
    for (uint32_t c = 0; c < 52u; c++)
        if (((c < 32u ? e.b.deck_lo >> c : e.b.deck_hi >> (c - 32u)) & 1u) != 0u) r_id[n++] = (uint8_t)c;
    for (; n < 64u; n++) r_id[n] = 0;
}

// Ranking: the word of the D-pair xy = qa | qb << 8 on the completion at D-positions pos[0..k) (unused entries 255), bd =
// mcq_exact_hero_board's.  A pair at or beyond n_rp (the padding of a row) is given as dead by the caller.
MCQ_HD uint32_t mcq_matrix_rank(const McqExactBoard &bd, const uint32_t pos[5], const uint8_t *r_id, uint32_t xy, const uint32_t *tf,
                                const uint32_t *tops, const uint32_t *sd) {
    const uint32_t qa = xy & 0xFFu, qb = xy >> 8;
    bool dead = false;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++) dead = dead || pos[i] == qa || pos[i] == qb;
    McqHole h;
    h.set(mcq_card(r_id[qa]), mcq_card(r_id[qb]));
    const uint32_t key = mcq_eval_key(bd.b, bd.fs, h, tf, tops, sd);
    return dead ? 0u : key + 1u;
}

/* the word as a column's: the dead mark above every live word */
MCQ_HD uint32_t mcq_matrix_col(uint32_t word) { return word != 0u ? word : 0xFFFFFFFFu; }

// Counting: one completion into a register tile.  row[TH]: the words of the tile's row hands, col[TG]: mcq_matrix_col of
// the words of its column hands.
template <uint32_t TH, uint32_t TG>
MCQ_HD void mcq_matrix_count(uint32_t (&cnt)[TH][TG], const uint32_t *row, const uint32_t *col) {
#pragma unroll
    for (uint32_t a = 0; a < TH; a++)
#pragma unroll
        for (uint32_t b = 0; b < TG; b++) cnt[a][b] += row[a] > col[b] ? 1u : 0u;
}

// Finish.  Per hand index (MCQ_HAND_INDEX, entries idx0, idx0 + step, ...): its cards a | b << 8 and its D-pair index, or
// MCQ_XM_NO_PAIR.  pos_of[52]: D-position of a card id, 255 = not in D.
MCQ_HD void mcq_matrix_pos_of(const McqMatrixQuery &e, const uint8_t *r_id, uint8_t *pos_of) {
    for (uint32_t c = 0; c < 52u; c++) pos_of[c] = 255;
    for (uint32_t i = 0; i < e.b.L; i++) pos_of[r_id[i]] = (uint8_t)i;
}
MCQ_HD void mcq_matrix_hands(const uint8_t *pos_of, uint32_t idx0, uint32_t step, uint16_t *cards, uint16_t *dpair) {
    for (uint32_t idx = idx0; idx < MCQ_XH_ROWS; idx += step) {
        uint32_t a, b;
        mcq_exact_pair_xy(idx, a, b);
        const uint32_t qa = pos_of[a], qb = pos_of[b];
        cards[idx] = (uint16_t)(a | (b << 8));
        dpair[idx] = qa == 255u || qb == 255u ? (uint16_t)MCQ_XM_NO_PAIR : (uint16_t)(qb * (qb - 1u) / 2u + qa);
    }
}
/* Entry (r, c): cnt = the counts by D-pair, [stride][stride].  The two hands can meet iff both lie in D and share no card. */
MCQ_HD void mcq_matrix_entry(const McqMatrixQuery &e, const uint16_t *cnt, uint32_t stride, const uint16_t *cards, const uint16_t *dpair,
                             uint32_t r, uint32_t c, uint32_t &win, uint32_t &tie) {
    const uint32_t i = dpair[r], j = dpair[c], hr = cards[r], hc = cards[c];
    const uint32_t ra = hr & 0xFFu, rb = hr >> 8, ca = hc & 0xFFu, cb = hc >> 8;
    const bool meet = i != MCQ_XM_NO_PAIR && j != MCQ_XM_NO_PAIR && ra != ca && ra != cb && rb != ca && rb != cb;
    win = tie = 0u;
    if (meet) {
        win = cnt[(size_t)i * stride + j];
        tie = e.total - win - cnt[(size_t)j * stride + i];
    }
}

#endif /* MCQ_EXACT_MATRIX_HPP */
