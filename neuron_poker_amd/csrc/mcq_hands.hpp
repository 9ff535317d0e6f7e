// mcq_hands.hpp -- the BLOCK TALLY PER HAND of mcq_eval_batch_ranges_hands (include/mcq.h): which hands of the watched
// seat's range carry its equity.  Plain integer code, written MCQ_HD: mcq_kernels.hip wires it to LDS and global atomics
// (mcq_eval_ranges_hands_kernel), tests/hostsim_ranges_hands walks it for the host in the kernel's block / round / wave
// order, tests/hostsim_ranges_hands/hs_main.cpp drives it on its own.
//
//   word layout   one table per BLOCK: MCQ_HAND_ROWS x 4 uint32 words (runs, win, tie, share), 21 KB of LDS; the words of
//                 hand h are those of mcq_hand_row h, so word w of the table belongs to 64-bit word w of the record's rows
//   add           what one iteration adds for the hand the watched seat held: one to runs and, when the seat is level
//                 with the best, one to win or tie and its share
//   piece         the tasks of a record that lie in a block's piece of the cost axis, dealt to the waves in rounds
//   flush bound   how many rounds a uint32 word holds
//   flush         table -> rows: every thread adds its non-zero words to the record's rows and clears them
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mcq_device.hpp"

// ---------------------------------------------------------------------------------------------- word layout
#define MCQ_HT_RUNS 0u
#define MCQ_HT_WIN 1u
#define MCQ_HT_TIE 2u
#define MCQ_HT_SHARE 3u
#define MCQ_HT_WORDS 4u
#define MCQ_HT_TABLE_WORDS (MCQ_HAND_ROWS * MCQ_HT_WORDS) /* 5304 words */
static_assert(sizeof(mcq_hand_row) == 8u * MCQ_HT_WORDS && offsetof(mcq_hand_row, runs) == 8u * MCQ_HT_RUNS &&
                  offsetof(mcq_hand_row, win) == 8u * MCQ_HT_WIN && offsetof(mcq_hand_row, tie) == 8u * MCQ_HT_TIE &&
                  offsetof(mcq_hand_row, share) == 8u * MCQ_HT_SHARE,
              "row of mcq_hand_row");

// ---------------------------------------------------------------------------------------------- add
/* hand: a | b << 8, a < b, as mcq_iteration_ranges keeps a seat's hand; level: the seat is one of the best hands; inc:
 * mcq_seat_increment of their number.  add(word, v): table[word] += v -- an LDS atomic on the device. */
template <class Add> MCQ_HD void mcq_hands_add(uint32_t hand, bool level, uint32_t inc, Add &add) {
    const uint32_t a = hand & 0xFFu, b = (hand >> 8) & 0xFFu;
    const uint32_t w = MCQ_HAND_INDEX(a, b) * MCQ_HT_WORDS;
    add(w + MCQ_HT_RUNS, 1u);
    if (level) {
        add(w + (((inc >> MCQ_SEAT_WIN_SHIFT) & 1u) ? MCQ_HT_WIN : MCQ_HT_TIE), 1u);
        add(w + MCQ_HT_SHARE, inc & 0xFFFFu);
    }
}
/* The lane accumulator of the per-hand entry: McqLaneAccSeats, and mcq_iteration_ranges hands every accepted iteration to
 * `dealt`, which adds the watched seat's hand to the block's table. */
template <class Add> struct McqLaneAccSeatsHands : McqLaneAccSeats {
    Add add;
    uint32_t watched; /* the seat, < n_players */
    MCQ_HDM void dealt(const uint16_t *ids, uint32_t ids_stride, uint32_t level, uint32_t inc) {
        mcq_hands_add(ids[watched * ids_stride], ((level >> watched) & 1u) != 0u, inc, add);
    }
};

// ---------------------------------------------------------------------------------------------- piece
/* A block owns [blo, bhi) of the cost axis.  Task t of a record that begins at pfx and prices a task at `weight` starts
 * at pfx + t * weight and belongs to the piece that holds its start (the rule of mcq_axis.hpp): the record's tasks
 * first .. end - 1 are the block's.  The waves of the block take them in rounds: wave v of `waves` runs task
 * first + round * waves + v, or nothing when that is not below end. */
struct McqHandsPiece {
    uint32_t first, end;
};
MCQ_HD McqHandsPiece mcq_hands_piece(uint64_t pfx, uint32_t weight, uint32_t n_tasks, uint64_t blo, uint64_t bhi) {
    uint64_t first = pfx < blo ? (blo - pfx - 1u) / weight + 1u : 0ull; /* (the tasks that start below blo; weight >= 1) */
    uint64_t end = pfx < bhi ? (bhi - pfx - 1u) / weight + 1u : 0ull;
    first = first < n_tasks ? first : n_tasks;
    end = end < n_tasks ? end : n_tasks;
    return {(uint32_t)first, (uint32_t)(end > first ? end : first)};
}
MCQ_HD uint32_t mcq_hands_rounds(const McqHandsPiece &p, uint32_t waves) { return (p.end - p.first + waves - 1u) / waves; }

// ---------------------------------------------------------------------------------------------- flush bound
/* A round is at most one task per wave: 16 waves x 64 lanes x MCQ_STREAM_ITERS iterations, each adding at most
 * MCQ_SHARE_UNIT to one word.  A uint32 word holds floor((2^32 - 1) / (16384 * 2520)) = 104 rounds; the table goes to
 * the rows after MCQ_HT_FLUSH_ROUNDS of them at the latest.  The waves of a block meet at every flush and nowhere
 * between two, so none is more than MCQ_HT_FLUSH_ROUNDS rounds ahead of the table's last clearing. */
#define MCQ_HT_BLOCK_WAVES 16u
#define MCQ_HT_ROUND_ITERS (MCQ_HT_BLOCK_WAVES * 64u * MCQ_STREAM_ITERS)
#define MCQ_HT_FLUSH_ROUNDS 64u
static_assert((uint64_t)MCQ_HT_FLUSH_ROUNDS * MCQ_HT_ROUND_ITERS * MCQ_SHARE_UNIT <= 0xFFFFFFFFull,
              "a table word holds the rounds between two flushes");
/* after `since` rounds without a flush, `left` rounds of the record's piece still to come: flush now?  (The end of a
 * piece flushes anyway.)  Block-uniform: both counts come from the piece alone. */
MCQ_HD bool mcq_hands_flush_due(uint32_t since, uint32_t left) { return since >= MCQ_HT_FLUSH_ROUNDS && left != 0u; }

// ---------------------------------------------------------------------------------------------- flush
/* Thread `thread` of `n_threads` takes words thread, thread + n_threads, ..: add(rows + w, v) for those that are not
 * zero -- a 64-bit global atomic on the device: other blocks hold parts of the same record -- and clears them.  Every
 * thread of the block calls it between two barriers. */
template <class Row, class Add64> MCQ_HD void mcq_hands_flush(uint32_t *table, uint32_t thread, uint32_t n_threads, Row *rows, Add64 add) {
    for (uint32_t w = thread; w < MCQ_HT_TABLE_WORDS; w += n_threads) {
        const uint32_t v = table[w];
        if (v != 0u) {
            add(rows + w, (Row)v);
            table[w] = 0u;
        }
    }
}
