// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the hero-range lane code
// (hs_hero_range.cpp), built and run under the host compiler's sanitizers by
// tests/test_hero_range_host.py::test_stand_alone_program_under_the_host_sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// One river and one turn case, both laws; prints the aggregates and returns 0 when every call was accepted.
#include <stdio.h>

#include "hs_hero_range.cpp"

static void all_classes(uint32_t *w) {
    for (int i = 0; i < 5; i++) w[i] = 0xFFFFFFFFu;
    w[5] = 0x1FFu;
}

int main() {
    std::vector<uint64_t> rows((size_t)MCQ_XH_ROWS * 13u);
    int bad = 0;
    for (int street = 0; street < 2; street++)
        for (int law = 0; law < 2; law++) {
            mcq_query q;
            mcq_query_ext x;
            memset(&q, 0, sizeof q);
            memset(&x, 0, sizeof x);
            const uint8_t river[5] = {4, 17, 22, 35, 44}, turn[4] = {51, 29, 10, 40};
            q.n_board = street == 0 ? 5 : 4;
            memcpy(q.board, street == 0 ? river : turn, q.n_board);
            q.n_players = 2;
            q.runs = 1;
            x.hero_is_range = 1;
            x.ghost[0] = x.ghost[1] = 0xFF;
            all_classes(x.hero_range);
            all_classes(x.opp_range);
            if (street == 1) { /* the turn: ghost cards, a restricted opponent (the pairs and the suited aces) */
                x.ghost[0] = 0;
                x.ghost[1] = 45;
                memset(x.opp_range, 0, sizeof x.opp_range);
                for (uint32_t r = 0; r < 13; r++) x.opp_range[(14u * r) >> 5] |= 1u << ((14u * r) & 31u);
                for (uint32_t r = 0; r < 12; r++) x.opp_range[(13u * r + 12u) >> 5] |= 1u << ((13u * r + 12u) & 31u);
            }
            double agg[11];
            const int rc = hs_hero_range(&q, &x, law, rows.data(), agg);
            uint64_t live = 0;
            for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) live += rows[13u * i] != 0;
            printf("%s law %d: rc %d, %llu hero hands, win %.9f tie %.9f\n", street == 0 ? "river" : "turn", law, rc,
                   (unsigned long long)live, agg[0], agg[1]);
            bad += rc != 0;
        }
    return bad;
}
