// hs_main.cpp -- TEST HARNESS ONLY: a stand-alone program around the host build of the dealing in epochs (hs_epochs.cpp),
// for a run under the host compiler's sanitizers:
//   g++ -O0 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined hs_main.cpp -o hs_main && ./hs_main
// (not optimised: inlined into one function per form, the instrumented lane code takes a minute to compile)
// The plans a lean build has (see hs_epochs.cpp; every rule), whole and stopped early, on rows that sit on the epoch
// boundaries and on random rows, against a plain list; then iterations of the forms a lean build has, and parity mode's.  Prints what it did and "ok: ..." as its last line; returns the number of failures.
#include <stdio.h>

#define HS_EPOCHS_LEAN 1
#include "hs_epochs.cpp"

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
    unsigned long long rows_checked = 0;
    for (int n_plan : {3, 7, 12, 15, 23})
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
            for (int rule : rules) {
                std::vector<uint8_t> pos(draws.size(), 0xEE);
                const int rc = hs_epochs_positions(n_plan, rule, n, draws.data(), rows, pos.data());
                if (rc != 0 || pos != want) {
                    printf("plan of %d draws, rule %d, %d dealt: rc %d, positions differ\n", n_plan, rule, n, rc);
                    bad++;
                }
                rows_checked += rows;
            }
        }
    printf("positions: %llu rows\n", rows_checked);

    int iterations = 0;
    for (int nopp = 1; nopp <= 9; nopp++)
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
            const int ndeal_known = 5 - nb;
            for (int known = 0; known < 2; known++) {
                if (known ? !((nopp == 1 && ndeal_known == 1) || (nopp == 5 && ndeal_known == 5)) : !(nopp == 5 || nopp == 9)) continue;
                for (int law = 0; law < 2; law++)
                    for (int ways = 0; ways < 2 - law; ways++) {
                        uint64_t a[22];
                        const int ra = hs_epochs_run(&q, 77, 5, nopp, known ? ndeal_known : -1, law, ways, 1, a);
                        uint64_t by_type = 0;
                        for (int t = 4; t < 13; t++) by_type += a[t];
                        if (ra || a[0] != 70 || a[1] != 70ull * (uint64_t)nopp || a[2] + a[3] != by_type || by_type > 70) {
                            printf("%d opponents, %d on the table, law %d, ways %d: rc %d, row does not add up\n", nopp, nb, law, ways, ra);
                            bad++;
                        }
                        iterations += 70;
                    }
            }
            uint64_t row[13];
            q.runs = 9; /* two loads of four iterations and a ragged one */
            const int rc = hs_epochs_replay(&q, 1234u + (uint32_t)nopp, row);
            if (rc || row[0] != 9 || row[2] + row[3] > 9 || row[1] < 9ull * (uint64_t)nopp) {
                printf("parity mode, %d opponents, %d on the table: rc %d\n", nopp, nb, rc);
                bad++;
            }
            iterations += 9;
        }
    printf("iterations: %d\n", iterations);
    printf("%s: %d failures\n", bad ? "FAILED" : "ok", bad);
    return bad;
}
