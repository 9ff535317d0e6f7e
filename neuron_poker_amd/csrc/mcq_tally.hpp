// mcq_tally.hpp -- WAVE TALLIES: how the lane accumulators of the Monte-Carlo kernels (McqLaneAcc, McqLaneAccWays,
// McqLaneAccSeats) become the 64-bit words of a result row.  Plain integer code, no HIP: mcq_kernels.hip wires it to its
// wave reductions and atomics, the host builds of the lane code (tests/hostsim*) fold their accumulators with it, and
// tests/hostsim_tally runs the lane states and the lanes -> row step for a simulated wave (tests/test_tally_host.py).
//
//   row layout   the words of mcq_result, mcq_result_ways and mcq_result_seats, held to include/mcq.h
//   fields       one function per packed field of an accumulator
//   fold         one accumulator into a row (what a wave does with 64 of them, without the wave)
//   lane states  McqTally, McqTallyWays, McqTallySeats: a lane's running sums between two flushes
//   lanes -> row the reduction is a template argument: lane l of the wave ends up holding word l + 1 of the row
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mcq_device.hpp"

// ---------------------------------------------------------------------------------------------- row layout
/* 64-bit words of a row; word 0 (runs) is written by the host or the prep kernels, never by a tally */
#define MCQ_RW_PASSES 1u
#define MCQ_RW_WIN 2u
#define MCQ_RW_TIE 3u
#define MCQ_RW_BY_TYPE 4u   /* + type, 9 words */
#define MCQ_RW_TIE_WAYS 13u /* + k - 2, MCQ_N_WAYS words (mcq_result_ways) */
#define MCQ_RW_SEAT 2u      /* + 3 * seat + MCQ_RW_SEAT_WIN / _TIE / _SHARE (mcq_result_seats) */
#define MCQ_RW_SEAT_WIN 0u
#define MCQ_RW_SEAT_TIE 1u
#define MCQ_RW_SEAT_SHARE 2u
#define MCQ_ROW_WORDS_PLAIN 13u
#define MCQ_ROW_WORDS_WAYS (MCQ_ROW_WORDS_PLAIN + MCQ_N_WAYS)
#define MCQ_ROW_WORDS_SEATS (MCQ_RW_SEAT + 3u * MCQ_MAX_SEATS)
#define MCQ_CODE_GAP 5u /* no hand has this code (mcq_code_to_type): its field of `types` is never counted */

static_assert(offsetof(mcq_result, passes) == 8u * MCQ_RW_PASSES && offsetof(mcq_result, win) == 8u * MCQ_RW_WIN &&
                  offsetof(mcq_result, tie) == 8u * MCQ_RW_TIE && offsetof(mcq_result, by_type) == 8u * MCQ_RW_BY_TYPE &&
                  sizeof(mcq_result) == 8u * MCQ_ROW_WORDS_PLAIN && MCQ_RW_BY_TYPE + (MCQ_N_CODES - 1u) == MCQ_ROW_WORDS_PLAIN,
              "row of mcq_result");
static_assert(offsetof(mcq_result_ways, r) == 0u && offsetof(mcq_result_ways, tie_ways) == 8u * MCQ_RW_TIE_WAYS &&
                  sizeof(mcq_result_ways) == 8u * MCQ_ROW_WORDS_WAYS,
              "row of mcq_result_ways");
static_assert(offsetof(mcq_result_seats, passes) == 8u * MCQ_RW_PASSES && offsetof(mcq_result_seats, seat) == 8u * MCQ_RW_SEAT &&
                  sizeof(mcq_result_seats) == 8u * MCQ_ROW_WORDS_SEATS && sizeof(mcq_seat) == 24u &&
                  offsetof(mcq_seat, win) == 8u * MCQ_RW_SEAT_WIN && offsetof(mcq_seat, tie) == 8u * MCQ_RW_SEAT_TIE &&
                  offsetof(mcq_seat, share) == 8u * MCQ_RW_SEAT_SHARE,
              "row of mcq_result_seats");

/* THE counter-to-word table: the word of code c's, way k's and seat s's counters; 0: the code is not counted */
MCQ_HD uint32_t mcq_row_code_word(uint32_t c) { return c == MCQ_CODE_GAP ? 0u : MCQ_RW_BY_TYPE + mcq_code_to_type(c); }
MCQ_HD uint32_t mcq_row_way_word(uint32_t k) { return MCQ_RW_TIE_WAYS + k; }
MCQ_HD uint32_t mcq_row_seat_word(uint32_t s, uint32_t field) { return MCQ_RW_SEAT + 3u * s + field; }
/* lanes -> row: lane l holds word l + 1 */
MCQ_HD bool mcq_row_owner(uint32_t lane, uint32_t word) { return lane == word - 1u; }

// ---------------------------------------------------------------------------------------------- fields
MCQ_HD uint32_t mcq_acc_code(uint64_t types, uint32_t c) { return (uint32_t)(types >> (6u * c)) & 63u; }      /* c = 0..9 */
MCQ_HD uint32_t mcq_acc_way(uint64_t ways, uint32_t k) { return (uint32_t)(ways >> (6u * (k + 1u))) & 63u; } /* k = 0..8 */
MCQ_HD uint32_t mcq_acc_seat_share(uint32_t w) { return w & 0xFFFFu; }
MCQ_HD uint32_t mcq_acc_seat_win(uint32_t w) { return (w >> MCQ_SEAT_WIN_SHIFT) & 31u; }
MCQ_HD uint32_t mcq_acc_seat_tie(uint32_t w) { return (w >> MCQ_SEAT_TIE_SHIFT) & 31u; }

// ---------------------------------------------------------------------------------------------- fold
/* one accumulator into a row: win = the codes' sum less the ties */
MCQ_HD uint64_t mcq_tally_fold_codes(uint64_t types, uint64_t *row) {
    uint64_t wins = 0;
    for (uint32_t c = 0; c < MCQ_N_CODES; c++) {
        if (!mcq_row_code_word(c)) continue;
        row[mcq_row_code_word(c)] += mcq_acc_code(types, c);
        wins += mcq_acc_code(types, c);
    }
    return wins;
}
MCQ_HD void mcq_tally_fold(const McqLaneAcc &a, uint64_t *row) {
    row[MCQ_RW_WIN] += mcq_tally_fold_codes(a.types, row) - a.tie;
    row[MCQ_RW_TIE] += a.tie;
    row[MCQ_RW_PASSES] += a.passes;
}
MCQ_HD void mcq_tally_fold(const McqLaneAccWays &a, uint64_t *row) { /* `tie` is the sum of the ways */
    uint64_t ties = 0;
    for (uint32_t k = 0; k < MCQ_N_WAYS; k++) {
        row[mcq_row_way_word(k)] += mcq_acc_way(a.ways, k);
        ties += mcq_acc_way(a.ways, k);
    }
    row[MCQ_RW_WIN] += mcq_tally_fold_codes(a.types, row) - ties;
    row[MCQ_RW_TIE] += ties;
    row[MCQ_RW_PASSES] += a.passes;
}
MCQ_HD void mcq_tally_fold(const McqLaneAccSeats &a, uint64_t *row) {
    row[MCQ_RW_PASSES] += a.passes;
    for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
        row[mcq_row_seat_word(s, MCQ_RW_SEAT_WIN)] += mcq_acc_seat_win(a.seat[s]);
        row[mcq_row_seat_word(s, MCQ_RW_SEAT_TIE)] += mcq_acc_seat_tie(a.seat[s]);
        row[mcq_row_seat_word(s, MCQ_RW_SEAT_SHARE)] += mcq_acc_seat_share(a.seat[s]);
    }
}

// ---------------------------------------------------------------------------------------------- lanes -> row
/* `sum(v)` is v added up over the 64 lanes of the wave, the same in every lane.  Packed forms put two counters into one
 * reduction as 16-bit halves; each is exact where the bound stated beside its use holds. */
#define MCQ_DIRECT_TASKS_LIMIT 32u /* most tasks of a query on the one-launch path: its row sums add two counters per word */
static_assert(64u * 16u * MCQ_DIRECT_TASKS_LIMIT < 65536u, "two counters per 32-bit reduction");
static_assert(64u * MCQ_STREAM_ITERS * MCQ_SHARE_UNIT < (1u << 22) && 64u * MCQ_STREAM_ITERS < 65536u,
              "a task's share in 22 bits, its win and tie as 16-bit halves");

/* The counters get(0 .. N-1) of a lane, in the words word(i) (0: not counted): the sum of their wave sums, and the wave
 * sum of the counter whose word the lane owns, or `mine` as it came. */
struct McqTallyPart {
    uint32_t total;
    uint64_t mine;
};
/* one reduction per counter, each picked up as it arrives ... */
template <uint32_t N, class Sum, class Get, class Word>
MCQ_HD McqTallyPart mcq_tally_counters(uint32_t lane, Sum &sum, Get get, Word word, uint64_t mine) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t i = 0; i < N; i++) {
        if (!word(i)) continue;
        const uint32_t v = sum(get(i));
        total += v;
        if (mcq_row_owner(lane, word(i))) mine = v;
    }
    return {total, mine};
}
/* ... or two counters per reduction (one that is not counted is zero), s[i] = the wave sum of counter i, picked up by
 * mcq_tally_pick once all reductions of the row have been issued */
template <uint32_t N, class Sum, class Get> MCQ_HD void mcq_tally_sums2(Sum &sum, Get get, uint32_t (&s)[N + 1u]) {
#pragma unroll
    for (uint32_t i = 0; i < N; i += 2) {
        const uint32_t hi = i + 1 < N ? get(i + 1) : 0u;
        const uint32_t v = sum(get(i) | (hi << 16));
        s[i] = v & 0xFFFFu;
        s[i + 1] = v >> 16;
    }
}
template <uint32_t N, class Word> MCQ_HD McqTallyPart mcq_tally_pick(uint32_t lane, const uint32_t (&s)[N + 1u], Word word, uint64_t mine) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t i = 0; i < N; i++) {
        if (!word(i)) continue;
        total += s[i];
        if (mcq_row_owner(lane, word(i))) mine = s[i];
    }
    return {total, mine};
}
MCQ_HD uint64_t mcq_tally_head(uint32_t lane, uint32_t pass, uint32_t wins, uint32_t ties, uint64_t mine) {
    if (mcq_row_owner(lane, MCQ_RW_PASSES)) mine = pass;
    if (mcq_row_owner(lane, MCQ_RW_WIN)) mine = wins - ties;
    if (mcq_row_owner(lane, MCQ_RW_TIE)) mine = ties;
    return mine;
}

// ---------------------------------------------------------------------------------------------- lane states
/* The evaluation kernels run at the register limit: the members and their widths are what the kernels can afford. */
struct McqTallyCodes { /* hero's winning codes (every iteration hero does not lose has one: their sum is the wins) */
    uint32_t code[MCQ_N_CODES];
    MCQ_HDM void add_codes(uint64_t types) {
#pragma unroll
        for (uint32_t c = 0; c < MCQ_N_CODES; c++)
            if (mcq_row_code_word(c)) code[c] += mcq_acc_code(types, c);
    }
    MCQ_HDM auto get_code() const {
        return [this](uint32_t c) { return code[c]; };
    }
    static MCQ_HDM uint32_t code_word(uint32_t c) { return mcq_row_code_word(c); }
};

struct McqTally : McqTallyCodes { /* per-lane running sums of the current (wave, query) pair */
    typedef McqLaneAcc Acc;
    static constexpr uint32_t kWords = MCQ_ROW_WORDS_PLAIN, kLanes = kWords - 1u;
    uint32_t tie, passes;
    bool dirty;
    MCQ_HDM void clear() {
#pragma unroll
        for (int c = 0; c < MCQ_N_CODES; c++) code[c] = 0;
        tie = passes = 0;
        dirty = false;
    }
    MCQ_HDM void add(const McqLaneAcc &a) {
        add_codes(a.types);
        tie += a.tie;
        passes += a.passes;
        dirty = true;
    }
    /* lane l < 12 returns word l + 1 of the row (passes, win, tie, by_type[9]) */
    template <class Sum> MCQ_HDM uint64_t row_value(uint32_t lane, Sum sum) const {
        const McqTallyPart wins = mcq_tally_counters<MCQ_N_CODES>(lane, sum, get_code(), code_word, 0);
        const uint32_t ties = sum(tie);
        const uint32_t pass = sum(passes);
        return mcq_tally_head(lane, pass, wins.total, ties, wins.mine);
    }
    /* the same for the one-launch path: the whole wave is active and a lane has added at most MCQ_DIRECT_TASKS_LIMIT tasks
     * of 16 iterations, so a counter's wave sum is below 2^16 and two counters share a reduction */
    template <class Sum> MCQ_HDM uint64_t row_words(uint32_t lane, Sum sum) const {
        uint32_t s[MCQ_N_CODES + 1];
        mcq_tally_sums2<MCQ_N_CODES>(sum, get_code(), s);
        const uint32_t ties = sum(tie);
        const uint32_t pass = sum(passes);
        const McqTallyPart wins = mcq_tally_pick<MCQ_N_CODES>(lane, s, code_word, 0);
        return mcq_tally_head(lane, pass, wins.total, ties, wins.mine);
    }
};

/* The split-pot rows (mcq_result_ways): tie_ways[k - 2] in word 13 + (k - 2) of the 22-word row, the same reductions and,
 * on the one-launch path, the same two-per-word packing.  The nine counters cost two registers more than the plain
 * tally, not nine: a lane keeps them as 10-bit fields, three per register -- a task adds at most 16 to a field, so the
 * tally is flushed after MCQ_WAYS_TALLY_TASKS tasks (the row's counters are atomic sums: a flush in the middle of a query
 * changes nothing) -- and `tie` is not kept at all: it is their sum. */
#define MCQ_WAYS_TALLY_TASKS 63u
struct McqTallyWays : McqTallyCodes {
    typedef McqLaneAccWays Acc;
    static constexpr uint32_t kWords = MCQ_ROW_WORDS_WAYS, kLanes = kWords - 1u;
    uint32_t passes, way3[3];
    uint32_t n_add; /* tasks added since the last flush (wave-uniform) */
    bool dirty;
    static_assert(16u * MCQ_WAYS_TALLY_TASKS < 1024u && MCQ_DIRECT_TASKS_LIMIT <= MCQ_WAYS_TALLY_TASKS, "10-bit fields");
    MCQ_HDM void clear() {
#pragma unroll
        for (int c = 0; c < MCQ_N_CODES; c++) code[c] = 0;
        way3[0] = way3[1] = way3[2] = 0;
        passes = 0;
        n_add = 0;
        dirty = false;
    }
    MCQ_HDM void add(const McqLaneAccWays &a) {
        add_codes(a.types);
#pragma unroll
        for (uint32_t k = 0; k < MCQ_N_WAYS; k++) way3[k / 3u] += mcq_acc_way(a.ways, k) << (10u * (k % 3u));
        passes += a.passes;
        n_add++;
        dirty = true;
    }
    MCQ_HDM bool full() const { return n_add >= MCQ_WAYS_TALLY_TASKS; }
    MCQ_HDM uint32_t way(uint32_t k) const { return (way3[k / 3u] >> (10u * (k % 3u))) & 1023u; }
    MCQ_HDM auto get_way() const {
        return [this](uint32_t k) { return way(k); };
    }
    static MCQ_HDM uint32_t way_word(uint32_t k) { return mcq_row_way_word(k); }
    template <class Sum> MCQ_HDM uint64_t row_value(uint32_t lane, Sum sum) const {
        const McqTallyPart wins = mcq_tally_counters<MCQ_N_CODES>(lane, sum, get_code(), code_word, 0);
        const McqTallyPart ties = mcq_tally_counters<MCQ_N_WAYS>(lane, sum, get_way(), way_word, wins.mine);
        const uint32_t pass = sum(passes);
        return mcq_tally_head(lane, pass, wins.total, ties.total, ties.mine);
    }
    template <class Sum> MCQ_HDM uint64_t row_words(uint32_t lane, Sum sum) const {
        uint32_t s_code[MCQ_N_CODES + 1], s_way[MCQ_N_WAYS + 1];
        mcq_tally_sums2<MCQ_N_CODES>(sum, get_code(), s_code);
        mcq_tally_sums2<MCQ_N_WAYS>(sum, get_way(), s_way);
        const uint32_t pass = sum(passes);
        const McqTallyPart wins = mcq_tally_pick<MCQ_N_CODES>(lane, s_code, code_word, 0);
        const McqTallyPart ties = mcq_tally_pick<MCQ_N_WAYS>(lane, s_way, way_word, wins.mine);
        return mcq_tally_head(lane, pass, wins.total, ties.total, ties.mine);
    }
};

/* The per-seat rows (mcq_result_seats, extended queries): word 1 passes, then win, tie, share of seat 0..9.  Thirty running
 * counters per lane would not fit beside the iteration's state, so nothing is kept per lane between tasks: a task's lane
 * words (McqLaneAccSeats: one packed word per seat) are summed over the wave at once -- the share field on its own, win
 * and tie together as 16-bit halves -- and every lane adds the sum of ITS word to one 64-bit register, which goes to the
 * row as one atomic per lane when the wave leaves the query. */
struct McqTallySeats {
    typedef McqLaneAccSeats Acc;
    static constexpr uint32_t kWords = MCQ_ROW_WORDS_SEATS, kLanes = kWords - 1u;
    uint64_t mine;
    bool dirty;
    MCQ_HDM void clear() {
        mine = 0;
        dirty = false;
    }
    template <class Sum> MCQ_HDM void add(const McqLaneAccSeats &a, uint32_t lane, Sum sum) { /* whole wave */
        const uint32_t pass = sum(a.passes);
        uint32_t v = mcq_row_owner(lane, MCQ_RW_PASSES) ? pass : 0u;
#pragma unroll
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
            const uint32_t w = a.seat[s];
            const uint32_t share = sum(mcq_acc_seat_share(w));
            const uint32_t wt = sum(mcq_acc_seat_win(w) | (mcq_acc_seat_tie(w) << 16)); /* (<= 1024 each) */
            v = mcq_row_owner(lane, mcq_row_seat_word(s, MCQ_RW_SEAT_WIN)) ? wt & 0xFFFFu : v;
            v = mcq_row_owner(lane, mcq_row_seat_word(s, MCQ_RW_SEAT_TIE)) ? wt >> 16 : v;
            v = mcq_row_owner(lane, mcq_row_seat_word(s, MCQ_RW_SEAT_SHARE)) ? share : v;
        }
        mine += v;
        dirty = true;
    }
    template <class Word, class Add> MCQ_HDM void flush(Word *row, uint32_t lane, Add add) {
        if (!dirty) return;
        if (lane < kLanes && mine != 0ull) add(row + 1 + lane, (Word)mine);
        clear();
    }
};
