// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the per-runout lane code
// (hs_runouts.cpp), for a run under the host compiler's sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// A turn with a known hand, a ranged opponent and ghost cards, and a flop all-in with three known hands (cases (b) and (c)
// of tests/runout_literal.py), both laws; prints the sums over the rows and returns 0 when every call was accepted and the
// rows add up as they must.
#include <stdio.h>

#include "hs_runouts.cpp"

static uint8_t id(const char *c) { /* "AS" -> 4 * rank + suit */
    const char *ranks = "23456789TJQKA", *suits = "CDHS";
    return (uint8_t)(4 * (int)(strchr(ranks, c[0]) - ranks) + (int)(strchr(suits, c[1]) - suits));
}
static void set_class(uint32_t *w, uint32_t bit) { w[bit >> 5] |= 1u << (bit & 31u); }

int main() {
    std::vector<uint64_t> cards((size_t)MCQ_XR_CARD_ROWS * MCQ_XR_WORDS), pairs((size_t)MCQ_XR_PAIR_ROWS * MCQ_XR_WORDS);
    int bad = 0;
    for (int which = 0; which < 2; which++)
        for (int law = 0; law < 2; law++) {
            mcq_query q;
            mcq_query_ext x;
            memset(&q, 0, sizeof q);
            memset(&x, 0, sizeof x);
            q.runs = 1;
            x.ghost[0] = x.ghost[1] = 0xFF;
            for (int i = 0; i < 5; i++) x.opp_range[i] = 0xFFFFFFFFu;
            x.opp_range[5] = 0x1FFu;
            if (which == 0) { /* the turn: KH QH on JH 9S 4D 4C, 9C 9D known, ghost AS 5C, opponent JJ / A4s / KQo */
                const char *b[4] = {"JH", "9S", "4D", "4C"};
                q.hole[0] = id("KH"); q.hole[1] = id("QH");
                for (int i = 0; i < 4; i++) q.board[i] = id(b[i]);
                q.n_board = 4;
                q.n_players = 3;
                x.n_known = 1;
                x.known[0].cards[0] = id("9C"); x.known[0].cards[1] = id("9D");
                x.ghost[0] = id("AS"); x.ghost[1] = id("5C");
                memset(x.opp_range, 0, sizeof x.opp_range);
                set_class(x.opp_range, 14u * 9u);       /* JJ */
                set_class(x.opp_range, 13u * 2u + 12u); /* A4 suited */
                set_class(x.opp_range, 13u * 11u + 10u); /* KQ off-suit */
            } else { /* the flop: AC KD on QS JH TC against AD KS, AH 2C and 9D 9H */
                const char *b[3] = {"QS", "JH", "TC"}, *k[3][2] = {{"AD", "KS"}, {"AH", "2C"}, {"9D", "9H"}};
                q.hole[0] = id("AC"); q.hole[1] = id("KD");
                for (int i = 0; i < 3; i++) q.board[i] = id(b[i]);
                q.n_board = 3;
                q.n_players = 4;
                x.n_known = 3;
                for (int h = 0; h < 3; h++) { x.known[h].cards[0] = id(k[h][0]); x.known[h].cards[1] = id(k[h][1]); }
            }
            const int rc = hs_runouts(&q, &x, law, cards.data(), pairs.data());
            uint64_t card_runs = 0, pair_runs = 0, live = 0;
            for (uint32_t c = 0; c < MCQ_XR_CARD_ROWS; c++) card_runs += cards[(size_t)c * MCQ_XR_WORDS];
            for (uint32_t p = 0; p < MCQ_XR_PAIR_ROWS; p++) { pair_runs += pairs[(size_t)p * MCQ_XR_WORDS]; live += pairs[(size_t)p * MCQ_XR_WORDS] != 0; }
            printf("%s law %d: rc %d, card rows hold %llu, pair rows %llu in %llu rows\n", which == 0 ? "turn" : "flop", law, rc,
                   (unsigned long long)card_runs, (unsigned long long)pair_runs, (unsigned long long)live);
            bad += rc != 0 || card_runs == 0 || (which == 0 ? pair_runs != 0 : card_runs != 2u * pair_runs);
        }
    return bad;
}
