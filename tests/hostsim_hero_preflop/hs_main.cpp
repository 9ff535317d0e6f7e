// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the preflop hero-range lane code
// (hs_hero_preflop.cpp), for a run under the host compiler's sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// Slices of the preflop enumeration at 52 and 50 cards (the first completions and the last ones, both laws, a narrow and
// an unrestricted hero range) and one flop through the generic form; returns 0 when every call was accepted.
#include <stdio.h>

#include "hs_hero_preflop.cpp"

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
    int bad = 0;
    for (int shape = 0; shape < 3; shape++)
        for (int law = 0; law < 2; law++) {
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
            if (shape == 1) { /* 50 cards, both ranges restricted, the last completions */
                x.ghost[0] = 50;
                x.ghost[1] = 51;
                pairs_and_suited_aces(x.hero_range);
                pairs_and_suited_aces(x.opp_range);
                hi = mcq_exact_binom(50u, 5u);
                lo = hi - 500u;
            }
            if (shape == 2) { /* a flop through the generic form: the whole enumeration, the aggregate */
                const uint8_t flop[3] = {51, 29, 10};
                q.n_board = 3;
                memcpy(q.board, flop, 3);
                pairs_and_suited_aces(x.opp_range);
                hi = 0xFFFFFFFFu;
            }
            double agg[11] = {0};
            uint32_t counts[4];
            const int rc = hs_hero_pre(&q, &x, law, lo, hi, rows.data(), agg, counts);
            uint64_t live = 0;
            for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) live += rows[13u * i] != 0;
            printf("shape %d law %d: rc %d, lists %u %u %u of %u completions, %llu rows with weight, win %.9f\n", shape, law, rc,
                   counts[0], counts[1], counts[2], counts[3], (unsigned long long)live, agg[0]);
            bad += rc != 0;
        }
    return bad;
}
