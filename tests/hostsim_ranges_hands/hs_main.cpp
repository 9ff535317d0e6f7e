// hs_main.cpp -- TEST HARNESS ONLY: the block tally per hand (neuron_poker_amd/csrc/mcq_hands.hpp) driven by a program of
// its own, which the tests build with AddressSanitizer and UndefinedBehaviorSanitizer: the first and the last hand of the
// table (the ends of its array), the flush bound with and without the rule, the pieces of a record on the cost axis.
// One line per case, then "ok: <cases>" or "FAILED".
#include <stdio.h>

#include "hs_hands.hpp"

int main() {
    unsigned cases = 0, failed = 0;
    auto report = [&](const char *what, bool ok) {
        printf("%s: %s\n", what, ok ? "holds" : "DIFFERS");
        cases++;
        failed += ok ? 0u : 1u;
    };
    const uint32_t win = mcq_seat_increment(1), tie3 = mcq_seat_increment(3);
    uint64_t row[4];
    uint32_t other = 0;
    {   /* the ends of the table: hand (0, 1) is row 0, hand (50, 51) is row 1325 */
        uint32_t fl = hs::drive(0, 1, win, 5, true, row, &other);
        report("first hand, five wins", fl == 0 && other == 0 && row[0] == 5 && row[1] == 5 && row[2] == 0 && row[3] == 5ull * MCQ_SHARE_UNIT);
        fl = hs::drive(50, 51, tie3, 7, true, row, &other);
        report("last hand, seven three-way ties", fl == 0 && other == 0 && row[0] == 7 && row[1] == 0 && row[2] == 7 && row[3] == 7ull * 840u);
    }
    {   /* a seat that is not level adds its run alone */
        std::vector<uint32_t> table(MCQ_HT_TABLE_WORDS, 0u);
        hs::TableAdd add = {table.data()};
        mcq_hands_add(3u | (9u << 8), false, win, add);
        const uint32_t w = MCQ_HAND_INDEX(3u, 9u) * MCQ_HT_WORDS;
        report("not level: runs alone", table[w] == 1 && table[w + 1] == 0 && table[w + 2] == 0 && table[w + 3] == 0);
    }
    {   /* the issue's count, 64 rounds and one add: the rule flushes once before the end, the row is exact */
        const uint64_t n = (uint64_t)MCQ_HT_FLUSH_ROUNDS * MCQ_HT_ROUND_ITERS + 1u;
        const uint32_t fl = hs::drive(48, 51, win, n, true, row, &other);
        report("64 rounds + 1 with the rule", fl == 1 && other == 0 && row[0] == n && row[1] == n && row[3] == n * MCQ_SHARE_UNIT);
    }
    {   /* 105 rounds: a uint32 word holds 104; with the rule exact, without it the share has wrapped */
        const uint64_t n = 105ull * MCQ_HT_ROUND_ITERS;
        uint32_t fl = hs::drive(48, 51, win, n, true, row, &other);
        report("105 rounds with the rule", fl == 1 && other == 0 && row[0] == n && row[3] == n * MCQ_SHARE_UNIT && row[3] > 0xFFFFFFFFull);
        fl = hs::drive(48, 51, win, n, false, row, &other);
        report("105 rounds without a flush wrap", fl == 0 && row[0] == n && row[3] == ((n * MCQ_SHARE_UNIT) & 0xFFFFFFFFull));
    }
    {   /* pieces: a record of 10 tasks of weight 7 at 100, cut at 121 (task 3 starts there) and at 135 (inside task 4) */
        McqHandsPiece p = mcq_hands_piece(100, 7, 10, 0, 121);
        bool ok = p.first == 0 && p.end == 3 && mcq_hands_rounds(p, 16) == 1;
        p = mcq_hands_piece(100, 7, 10, 121, 135);
        ok = ok && p.first == 3 && p.end == 5 && mcq_hands_rounds(p, 1) == 2;
        p = mcq_hands_piece(100, 7, 10, 135, 1000);
        ok = ok && p.first == 5 && p.end == 10 && mcq_hands_rounds(p, 4) == 2;
        p = mcq_hands_piece(100, 7, 10, 170, 1000); /* behind the record */
        ok = ok && p.first == p.end && mcq_hands_rounds(p, 16) == 0;
        p = mcq_hands_piece(100, 7, 10, 0, 100); /* in front of it */
        ok = ok && p.first == p.end;
        p = mcq_hands_piece(0, 0xFFFFFFFFu, 0x400000u, 0, ~0ull); /* the largest weight and task count */
        ok = ok && p.first == 0 && p.end == 0x400000u;
        report("pieces of a record", ok);
    }
    if (failed) printf("FAILED: %u of %u\n", failed, cases);
    else printf("ok: %u\n", cases);
    return failed ? 1 : 0;
}
