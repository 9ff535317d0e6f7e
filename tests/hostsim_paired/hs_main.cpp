// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the paired count (hs_paired.cpp), for a
// run under the host compiler's sanitizers:
//   g++ -O0 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// (not optimised: inlined into one function per form, the instrumented lane code takes a minute to compile)
// The primitive on every byte pair; the plans a lean build has (see hs_paired.cpp; every rule, the switch on and off), whole
// and stopped early, on rows that sit on the epoch boundaries and on random rows, against a plain list; then iterations of
// the forms a lean build has, switch on against switch off, and parity mode's.  Prints what it did and "ok: ..." as its last
// line; returns the number of failures.
#include <stdio.h>

#define HS_PAIRED_LEAN 1
#include "hs_paired.cpp"

static uint32_t g_rng = 0x9E3779B9u;
static uint32_t rnd() { /* xorshift32 */
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

static void list_pop(const uint8_t *r, int n, int deck_len, uint8_t *pos) {
    uint8_t deck[64];
    for (int i = 0; i < deck_len; i++) deck[i] = (uint8_t)i;
    int len = deck_len;
    for (int j = 0; j < n; j++) {
        pos[j] = deck[r[j]];
        for (int i = r[j]; i + 1 < len; i++) deck[i] = deck[i + 1];
        len--;
    }
}

int main() {
    const int rules[4] = {1, 2, 3, MCQ_DEAL_FULLREG};
    int bad = 0;

    /* the primitive: every p against every pair of bytes a plain and a biased register can hold (a coordinate 0..49, a free
     * slot moved down by 0..13 scans), in every byte lane, the other lanes free slots */
    unsigned long long pairs_checked = 0;
    for (uint32_t p = 0; p < 50; p++)
        for (uint32_t a = 0; a < 64; a++)
            for (uint32_t b = 0; b < 64; b++) {
                const uint32_t ta = a < 50 ? a : 0x7Fu - (a - 50), tb = b < 50 ? b + 0x40u : 0x7Fu - (b - 50);
                for (uint32_t lane = 0; lane < 4; lane++) {
                    const uint32_t sh = 8u * lane, pb = (p | 0x80u) * 0x01010101u;
                    const uint32_t h0 = (MCQ_HOLE_SENTINEL & ~(0xFFu << sh)) | (ta << sh);
                    const uint32_t h1b = ((MCQ_HOLE_SENTINEL - 0x03030303u) & ~(0xFFu << sh)) | (tb << sh);
                    uint32_t got, single;
                    hs_paired_count2(1, &pb, &h0, &h1b, &got, &single);
                    const uint32_t want = (a < 50 && a <= p ? 1u : 0u) + (b < 50 && b <= p ? 1u : 0u);
                    if (got != want || single != want) {
                        if (bad < 10) printf("count2: p %u, bytes %02x %02x, lane %u: %u (singly %u), want %u\n", p, ta, tb, lane, got, single, want);
                        bad++;
                    }
                    pairs_checked++;
                }
            }
    printf("primitive: %llu registers\n", pairs_checked);

    unsigned long long rows_checked = 0;
    for (int n_plan : {7, 12, 15, 19, 23})
        for (int n = (n_plan > 5 ? n_plan - 5 : 1); n <= n_plan; n++) {
            const int deck_len = 50 - (n_plan - n > 5 ? 5 : n_plan - n); /* n_plan - n table cards are already known */
            std::vector<uint8_t> draws, want;
            auto add_row = [&](auto value) {
                for (int j = 0; j < n; j++) {
                    int v = value(j), top = deck_len - 1 - j;
                    draws.push_back((uint8_t)(v < 0 ? 0 : v > top ? top : v));
                }
            };
            add_row([](int) { return 0; });
            add_row([](int) { return 99; });          /* the last index of every list */
            add_row([](int j) { return j; });
            add_row([&](int j) { return n - 1 - j; });
            for (int j0 = 1; j0 < n; j0++)
                for (int d = -1; d <= 1; d++) add_row([&](int j) { return 6 + (j >= j0 ? d : 0); });
            for (int k = 0; k < 200; k++) add_row([&](int j) { return (int)(rnd() % (uint32_t)(deck_len - j)); });
            const uint64_t rows = draws.size() / (size_t)n;
            want.resize(draws.size());
            for (uint64_t i = 0; i < rows; i++) list_pop(&draws[i * n], n, deck_len, &want[i * n]);
            for (int rule : rules)
                for (int paired = 0; paired < 2; paired++) {
                    std::vector<uint8_t> pos(draws.size(), 0xEE);
                    const int rc = hs_paired_positions(n_plan, rule, paired, n, draws.data(), rows, pos.data());
                    if (rc != 0 || pos != want) {
                        printf("plan of %d draws, rule %d, paired %d, %d dealt: rc %d, positions differ\n", n_plan, rule, paired, n, rc);
                        bad++;
                    }
                    rows_checked += rows;
                }
        }
    printf("positions: %llu rows\n", rows_checked);

    int iterations = 0;
    for (int nopp : {5, 7, 9})
        for (int nb : {0, 3, 4, 5}) {
            mcq_query q;
            memset(&q, 0, sizeof q);
            q.hole[0] = (uint8_t)(2 * nopp + 3);
            q.hole[1] = (uint8_t)(36 + nopp);
            const uint8_t table[5] = {30, 34, 1, 47, 16};
            for (int i = 0; i < nb; i++) q.board[i] = table[i];
            for (int i = nb; i < 5; i++) q.board[i] = 0xFF;
            q.n_board = (uint8_t)nb;
            q.n_players = (uint8_t)(nopp + 1);
            q.runs = 70;
            for (int known = 0; known < 2; known++) {
                if (known && !(nopp == 5 && nb == 0)) continue;
                uint64_t a[13], b[13];
                const int ra = hs_paired_run(&q, 77, 5, nopp, known ? 5 : -1, 0, 0, 1, a);
                const int rb = hs_paired_run(&q, 77, 5, nopp, known ? 5 : -1, 0, 0, 0, b);
                uint64_t by_type = 0;
                for (int t = 4; t < 13; t++) by_type += a[t];
                if (ra || rb || memcmp(a, b, sizeof a) != 0 || a[0] != 70 || a[1] != 70ull * (uint64_t)nopp || a[2] + a[3] != by_type || by_type > 70) {
                    printf("%d opponents, %d on the table: rc %d %d, rows differ or do not add up\n", nopp, nb, ra, rb);
                    bad++;
                }
                iterations += 140;
            }
            if (nopp == 5) {
                uint64_t row[13];
                q.runs = 9; /* two loads of four iterations and a ragged one */
                const int rc = hs_paired_replay(&q, 1234u + (uint32_t)nb, row);
                if (rc || row[0] != 9 || row[2] + row[3] > 9 || row[1] < 9ull * (uint64_t)nopp) {
                    printf("parity mode, %d opponents, %d on the table: rc %d\n", nopp, nb, rc);
                    bad++;
                }
                iterations += 9;
            }
        }
    printf("iterations: %d\n", iterations);
    printf("%s: %d failures\n", bad ? "FAILED" : "ok", bad);
    return bad;
}
