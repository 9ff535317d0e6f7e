// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the weighted preflop hero-range lane
// code (hs_hero_preflop_weighted.cpp), for a run under the host compiler's sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// Slices of the preflop enumeration at 52 cards (every class, an opponent table alone, the first completions) and at 50
// cards (ghost cards, both ranges restricted, a hero table with zeros, the last completions) and one whole turn through the
// generic form; the tables are opp[i] = i % 3 ? (i * 40503) & 0xFFFF : 0 and hero[i] = i % 5 ? 1 + i % 7 : 0.  Prints per
// case the list counts, the hero hands with a row, the sum of their runs and the aggregate's win, and returns 0 when every
// call was accepted.
#include <stdio.h>

#include "hs_hero_preflop_weighted.cpp"

static void all_classes(uint32_t *w) {
    for (int i = 0; i < 5; i++) w[i] = 0xFFFFFFFFu;
    w[5] = 0x1FFu;
}
static void pairs_and_suited_aces(uint32_t *w) {
    memset(w, 0, 24);
    for (uint32_t r = 0; r < 13; r++) w[(14u * r) >> 5] |= 1u << ((14u * r) & 31u);
    for (uint32_t r = 0; r < 12; r++) w[(13u * r + 12u) >> 5] |= 1u << ((13u * r + 12u) & 31u);
}

int main() {
    std::vector<uint64_t> rows((size_t)MCQ_XH_ROWS * 13u);
    std::vector<uint16_t> opp(MCQ_XH_ROWS), hero(MCQ_XH_ROWS);
    for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) {
        opp[i] = (uint16_t)(i % 3u ? (i * 40503u) & 0xFFFFu : 0u);
        hero[i] = (uint16_t)(i % 5u ? 1u + i % 7u : 0u);
    }
    int bad = 0;
    for (int shape = 0; shape < 3; shape++) {
        mcq_query q;
        mcq_query_ext x;
        memset(&q, 0, sizeof q);
        memset(&x, 0, sizeof x);
        q.n_players = 2;
        q.runs = 1;
        x.hero_is_range = 1;
        x.ghost[0] = x.ghost[1] = 0xFF;
        all_classes(x.hero_range);
        all_classes(x.opp_range);
        uint32_t lo = 0, hi = 40;
        const uint16_t *hw = nullptr;
        if (shape == 1) { /* 50 cards, both ranges restricted, hero weights with zeros, the last completions */
            x.ghost[0] = 50;
            x.ghost[1] = 51;
            pairs_and_suited_aces(x.hero_range);
            pairs_and_suited_aces(x.opp_range);
            hw = hero.data();
            hi = mcq_exact_binom(50u, 5u);
            lo = hi - 500u;
        }
        if (shape == 2) { /* a turn through the generic form: the whole enumeration, the aggregate */
            const uint8_t turn[4] = {51, 29, 10, 40};
            q.n_board = 4;
            memcpy(q.board, turn, 4);
            x.ghost[0] = 0;
            x.ghost[1] = 45;
            pairs_and_suited_aces(x.opp_range);
            hw = hero.data();
            hi = 0xFFFFFFFFu;
        }
        double agg[11] = {0};
        uint32_t counts[4] = {0, 0, 0, 0};
        const int rc = hs_hero_pre_w(&q, &x, opp.data(), hw, lo, hi, rows.data(), agg, counts);
        uint64_t live = 0, runs = 0;
        for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) {
            live += rows[13u * i] != 0;
            runs += rows[13u * i];
        }
        printf("shape %d: rc %d, lists %u %u %u of %u completions, %llu hero hands, runs %llu, win %.9f\n", shape, rc, counts[0],
               counts[1], counts[2], counts[3], (unsigned long long)live, (unsigned long long)runs, agg[0]);
        bad += rc != 0;
    }
    return bad;
}
