// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the opponents' cards read by flush suit
// (hs_bysuit.cpp), for a run under the host compiler's sanitizers:
//   g++ -O0 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// The hole tables of a few base decks, filled by put_holes and read back at every position and suit in both layouts (each
// table ends its heap block: a store or a read behind position 49 stops the program), then iterations of the forms a lean
// build has through every accessor, which must give the rows of the cards read where they are dealt.  Prints what it did
// and "ok: ..." as its last line; returns the number of failures.
#include <stdio.h>

#define HS_BYSUIT_LEAN 1
#include "hs_bysuit.cpp"

int main() {
    int bad = 0, decks = 0, iterations = 0;
    const uint8_t table[5] = {30, 34, 38, 47, 16}; /* 9H TH JH KS 6C */
    for (int nb : {0, 3, 4, 5})
        for (int suited = 0; suited < 2; suited++) {
            mcq_query q;
            memset(&q, 0, sizeof q);
            q.hole[0] = 50;
            q.hole[1] = (uint8_t)(suited ? 46 : 45);
            for (int i = 0; i < 5; i++) q.board[i] = i < nb ? table[i] : 0xFF;
            q.n_board = (uint8_t)nb;
            q.n_players = 6;
            q.runs = 1;
            std::vector<uint32_t> e(5u * MCQ_HOLE_POSITIONS * 4u * 2u, 0xEEEEEEEEu);
            const int n = hs_bysuit_entries(&q, e.data());
            const size_t per = MCQ_HOLE_POSITIONS * 4u * 2u;
            if (n != 50 - nb) { printf("%d table cards: hs_bysuit_entries %d\n", nb, n); bad++; continue; }
            for (int k = 1; k < 5; k++)
                if (memcmp(&e[0], &e[k * per], per * sizeof(uint32_t)) != 0) {
                    printf("%d table cards, suited %d: source %d differs from set + perm\n", nb, suited, k);
                    bad++;
                }
            decks++;
        }
    printf("decks: %d\n", decks);

    for (int nopp : {1, 5, 9})
        for (int nb : {0, 3, 4, 5}) {
            mcq_query q;
            memset(&q, 0, sizeof q);
            q.hole[0] = (uint8_t)(2 * nopp + 3);
            q.hole[1] = (uint8_t)(36 + nopp);
            for (int i = 0; i < 5; i++) q.board[i] = i < nb ? table[i] : 0xFF;
            q.n_board = (uint8_t)nb;
            q.n_players = (uint8_t)(nopp + 1);
            q.runs = 70;
            const int ndeal_known = 5 - nb;
            for (int known = 0; known < 2; known++) {
                if (known ? !((nopp == 1 && ndeal_known == 1) || (nopp == 5 && ndeal_known == 5)) : !(nopp == 5 || nopp == 9)) continue;
                for (int law = 0; law < 2; law++)
                    for (int ways = 0; ways < 2 - law; ways++) {
                        uint64_t want[22], got[22];
                        const int nd = known ? ndeal_known : -1;
                        int rc = hs_bysuit_run(&q, 77, 5, nopp, nd, law, ways, 0, want);
                        if (rc || want[0] != 70 || want[1] != 70ull * (uint64_t)nopp || want[2] + want[3] > 70) {
                            printf("%d opponents, %d on the table, law %d, ways %d: rc %d, row does not add up\n", nopp, nb, law, ways, rc);
                            bad++;
                        }
                        for (int accessor = 1; accessor <= 3; accessor++) {
                            rc = hs_bysuit_run(&q, 77, 5, nopp, nd, law, ways, accessor, got);
                            if (rc || memcmp(got, want, (ways ? 22 : 13) * sizeof(uint64_t)) != 0) {
                                printf("%d opponents, %d on the table, law %d, ways %d, accessor %d: rc %d, rows differ\n", nopp, nb,
                                       law, ways, accessor, rc);
                                bad++;
                            }
                            iterations += 70;
                        }
                    }
            }
        }
    printf("iterations: %d\n", iterations);
    printf("%s: %d failures\n", bad ? "FAILED" : "ok", bad);
    return bad;
}
