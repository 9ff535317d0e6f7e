// hs_hands.hpp -- TEST HARNESS ONLY: the block tally per hand (neuron_poker_amd/csrc/mcq_hands.hpp) for the host compiler,
// with the host's forms of its two adds, and the driver of the flush bound that hs_ranges_hands.cpp (a library the tests
// load) and hs_main.cpp (a program the tests run under the sanitizers) share.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_hands.hpp"

namespace hs {
/* the table's add: a uint32 word that wraps as the LDS word does */
struct TableAdd {
    uint32_t *table;
    void operator()(uint32_t word, uint32_t v) const { table[word] += v; }
};
/* the rows' add */
struct RowAdd {
    void operator()(uint64_t *word, uint64_t v) const { *word += v; }
};
/* every thread of a block of n_threads flushes, one behind the other */
inline void flush(std::vector<uint32_t> &table, uint32_t n_threads, uint64_t *rows) {
    for (uint32_t t = 0; t < n_threads; t++) mcq_hands_flush(table.data(), t, n_threads, rows, RowAdd());
}

/* One hand (a, b) takes `inc` (an mcq_seat_increment word) n_adds times, no iteration dealt: the adds come in rounds of
 * MCQ_HT_ROUND_ITERS, and behind each round the kernel's rule decides about a flush (with_flush) or nothing is flushed
 * before the end.  row: the hand's four 64-bit words.  -> the number of flushes before the end; other_words (may be null):
 * how many words of other hands are not zero in the table or the rows at the end. */
inline uint32_t drive(uint32_t a, uint32_t b, uint32_t inc, uint64_t n_adds, bool with_flush, uint64_t *row, uint32_t *other_words) {
    std::vector<uint32_t> table(MCQ_HT_TABLE_WORDS, 0u);
    std::vector<uint64_t> rows(MCQ_HT_TABLE_WORDS, 0ull);
    TableAdd add = {table.data()};
    const uint64_t rounds = (n_adds + MCQ_HT_ROUND_ITERS - 1u) / MCQ_HT_ROUND_ITERS;
    uint32_t since = 0, flushes = 0;
    uint64_t done = 0;
    for (uint64_t r = 0; r < rounds; r++) {
        for (uint32_t k = 0; k < MCQ_HT_ROUND_ITERS && done < n_adds; k++, done++) mcq_hands_add(a | (b << 8), true, inc, add);
        since++;
        const uint64_t left = rounds - 1u - r;
        if (with_flush && mcq_hands_flush_due(since, left > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)left)) {
            flush(table, 64u * MCQ_HT_BLOCK_WAVES, rows.data());
            since = 0;
            flushes++;
        }
    }
    flush(table, 64u * MCQ_HT_BLOCK_WAVES, rows.data());
    const uint32_t w0 = MCQ_HAND_INDEX(a, b) * MCQ_HT_WORDS;
    uint32_t other = 0;
    for (uint32_t w = 0; w < MCQ_HT_TABLE_WORDS; w++) {
        if (w >= w0 && w < w0 + MCQ_HT_WORDS) row[w - w0] = rows[w];
        else other += rows[w] != 0ull ? 1u : 0u;
        other += table[w] != 0u ? 1u : 0u; /* (a flush leaves the table clear) */
    }
    if (other_words) *other_words = other;
    return flushes;
}
}  // namespace hs
