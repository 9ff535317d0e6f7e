// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the weighted hero-range lane code
// (hs_hero_weighted.cpp), for a run under the host compiler's sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// One river (every class, an opponent table alone) and one turn (ghost cards, a restricted opponent, a hero table with
// zeros); the tables are opp[i] = i % 3 ? (i * 40503) & 0xFFFF : 0 and hero[i] = i % 5 ? 1 + i % 7 : 0.  Prints per case
// the hero hands with a row, the sum of their runs and the aggregate, and returns 0 when every call was accepted.
#include <stdio.h>

#include "hs_hero_weighted.cpp"

static void all_classes(uint32_t *w) {
    for (int i = 0; i < 5; i++) w[i] = 0xFFFFFFFFu;
    w[5] = 0x1FFu;
}

int main() {
    std::vector<uint64_t> rows((size_t)MCQ_XH_ROWS * 13u);
    std::vector<uint16_t> opp(MCQ_XH_ROWS), hero(MCQ_XH_ROWS);
    for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) {
        opp[i] = (uint16_t)(i % 3u ? (i * 40503u) & 0xFFFFu : 0u);
        hero[i] = (uint16_t)(i % 5u ? 1u + i % 7u : 0u);
    }
    int bad = 0;
    for (int street = 0; street < 2; street++) {
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
        const int rc = hs_hero_weighted(&q, &x, opp.data(), street == 1 ? hero.data() : nullptr, rows.data(), agg);
        uint64_t live = 0, runs = 0;
        for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) {
            live += rows[13u * i] != 0;
            runs += rows[13u * i];
        }
        printf("%s: rc %d, %llu hero hands, runs %llu, win %.9f tie %.9f\n", street == 0 ? "river" : "turn", rc,
               (unsigned long long)live, (unsigned long long)runs, agg[0], agg[1]);
        bad += rc != 0;
    }
    return bad;
}
