// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the matrix lane code (hs_matrix.cpp), built
// and run under the host compiler's sanitizers by tests/test_matrix_host.py::test_stand_alone_program_under_the_host_sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// A river, a turn with two dead cards, a flop with 43 dead cards (six cards left: one partial tile) and a refused record;
// prints per case the return code, total and the sums of both matrices, and returns 0 when the three were accepted and the
// fourth refused.
#include <stdio.h>

#include "hs_matrix.cpp"

int main() {
    std::vector<uint16_t> win((size_t)MCQ_XH_ROWS * MCQ_XH_ROWS), tie((size_t)MCQ_XH_ROWS * MCQ_XH_ROWS);
    const uint8_t river[5] = {4, 17, 22, 35, 44}, turn[4] = {51, 29, 10, 40}, flop[3] = {50, 46, 21};
    int bad = 0;
    for (int i = 0; i < 4; i++) {
        mcq_matrix_query q;
        memset(&q, 0, sizeof q);
        q.n_board = i == 0 ? 5 : i == 1 ? 4 : 3;
        memcpy(q.board, i == 0 ? river : i == 1 ? turn : flop, q.n_board);
        if (i == 1) q.dead = (1ull << 0) | (1ull << 45);
        if (i >= 2) { /* the lowest cards that are not on the table: 43 of them, then 45 */
            uint32_t n = 0;
            for (uint32_t c = 0; c < 52u && n < (i == 2 ? 43u : 45u); c++)
                if (c != 50u && c != 46u && c != 21u) {
                    q.dead |= 1ull << c;
                    n++;
                }
        }
        uint32_t total = 0;
        const int rc = hs_matrix(&q, win.data(), tie.data(), &total);
        unsigned long long sw = 0, st = 0;
        if (rc == 0)
            for (size_t j = 0; j < win.size(); j++) {
                sw += win[j];
                st += tie[j];
            }
        printf("case %d: rc %d, total %u, win %llu, tie %llu\n", i, rc, total, sw, st);
        bad += i < 3 ? rc != 0 : rc != MCQ_XM_SHORT;
    }
    return bad;
}
