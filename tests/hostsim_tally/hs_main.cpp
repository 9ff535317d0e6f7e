// hs_main.cpp -- TEST HARNESS ONLY: the cases of tests/test_tally_host.py walked by a program of its own, which the tests
// build with AddressSanitizer and UndefinedBehaviorSanitizer.  One line per case, then "ok: <cases>" or "FAILED".
#include <stdio.h>

#include "hs_tally.hpp"

namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) { /* 0 .. n-1 */
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}
/* a legal record of `kind`: sixteen iterations, each lost or won with a code and e opponents sharing the pot; the
 * per-seat kind: k of ten seats best */
void legal(uint32_t kind, uint64_t *r) {
    memset(r, 0, hs::kRec * sizeof(uint64_t));
    for (uint32_t it = 0; it < MCQ_STREAM_ITERS; it++) {
        if (kind == 2) {
            const uint32_t k = 1u + rnd(MCQ_MAX_SEATS), first = rnd(MCQ_MAX_SEATS);
            for (uint32_t j = 0; j < k; j++) r[1 + (first + j) % MCQ_MAX_SEATS] += mcq_seat_increment(k);
            continue;
        }
        if (rnd(3) == 0) continue;
        uint32_t c = rnd(MCQ_N_CODES - 1u);
        c += c >= MCQ_CODE_GAP ? 1u : 0u;
        const uint32_t e = rnd(4) ? 0u : 1u + rnd(MCQ_N_WAYS);
        r[0] += 1ull << (6u * c);
        if (kind == 0) r[1] += e ? 1u : 0u;
        else r[2] += 1ull << (6u * e);
    }
    r[kind == 0 ? 2 : kind == 1 ? 1 : 0] = rnd(1000);
}
/* every field at its largest: 16 */
void largest(uint32_t kind, uint64_t *r) {
    memset(r, 0, hs::kRec * sizeof(uint64_t));
    if (kind == 2) {
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) r[1 + s] = 16u * MCQ_SHARE_UNIT | 16u << MCQ_SEAT_WIN_SHIFT | 16u << MCQ_SEAT_TIE_SHIFT;
        return;
    }
    for (uint32_t c = 0; c < MCQ_N_CODES; c++) r[0] |= 16ull << (6u * c);
    if (kind == 0) r[1] = 16;
    else for (uint32_t e = 0; e <= MCQ_N_WAYS; e++) r[2] |= 16ull << (6u * e);
}
bool wave_is_fold(uint32_t kind, bool packed, const std::vector<uint64_t> &recs, uint32_t tasks) {
    uint64_t row[32] = {}, words[hs::kWave] = {};
    bool ok;
    uint32_t lanes;
    if (kind == 0) {
        hs::fold<McqLaneAcc>(recs.data(), (uint64_t)tasks * hs::kWave, row);
        ok = hs::wave_words<McqTally>(recs.data(), tasks, packed, words);
        lanes = McqTally::kLanes;
    } else if (kind == 1) {
        hs::fold<McqLaneAccWays>(recs.data(), (uint64_t)tasks * hs::kWave, row);
        ok = hs::wave_words<McqTallyWays>(recs.data(), tasks, packed, words);
        lanes = McqTallyWays::kLanes;
    } else {
        McqTallySeats st[hs::kWave];
        hs::fold<McqLaneAccSeats>(recs.data(), (uint64_t)tasks * hs::kWave, row);
        ok = hs::wave_seats(st, recs.data(), tasks);
        for (uint32_t l = 0; l < hs::kWave; l++) words[l] = st[l].mine;
        lanes = McqTallySeats::kLanes;
    }
    for (uint32_t l = 0; l < hs::kWave; l++) ok = ok && words[l] == (l < lanes ? row[1 + l] : 0u);
    return ok;
}
}  // namespace

int main() {
    unsigned cases = 0, failed = 0;
    auto report = [&](const char *what, uint32_t kind, bool ok) {
        printf("%s, kind %u: %s\n", what, kind, ok ? "holds" : "DIFFERS");
        cases++;
        failed += ok ? 0u : 1u;
    };
    for (uint32_t kind = 0; kind < 3; kind++) {
        for (int packed = 0; packed < (kind == 2 ? 1 : 2); packed++) { /* random lanes, a random number of tasks each */
            const uint32_t tasks = packed ? MCQ_DIRECT_TASKS_LIMIT : MCQ_WAYS_TALLY_TASKS;
            std::vector<uint64_t> recs((size_t)tasks * hs::kWave * hs::kRec, 0);
            for (uint32_t l = 0; l < hs::kWave; l++)
                for (uint32_t t = 0, n = 1u + rnd(tasks); t < n; t++) legal(kind, &recs[((size_t)t * hs::kWave + l) * hs::kRec]);
            report(packed ? "wave against fold, two per reduction" : "wave against fold", kind, wave_is_fold(kind, packed != 0, recs, tasks));
        }
        for (int packed = 0; packed < (kind == 2 ? 1 : 2); packed++) { /* every field at 16 in every lane up to the task limit */
            const uint32_t tasks = packed || kind == 2 ? MCQ_DIRECT_TASKS_LIMIT : MCQ_WAYS_TALLY_TASKS;
            std::vector<uint64_t> recs((size_t)tasks * hs::kWave * hs::kRec);
            for (size_t i = 0; i < (size_t)tasks * hs::kWave; i++) largest(kind, &recs[i * hs::kRec]);
            report(packed || kind == 2 ? "largest fields, 16-bit halves" : "largest fields, 63 tasks", kind, wave_is_fold(kind, packed != 0, recs, tasks));
        }
    }
    { /* the 10-bit fields: full after 63 tasks, exact until then, a 64th carries into the neighbour */
        uint64_t r[hs::kRec];
        largest(1, r);
        McqTallyWays t;
        t.clear();
        bool ok = true;
        for (uint32_t i = 1; i <= MCQ_WAYS_TALLY_TASKS; i++) {
            McqLaneAccWays a;
            hs::acc_of(r, a);
            t.add(a);
            ok = ok && t.full() == (i == MCQ_WAYS_TALLY_TASKS) && t.way(0) == 16u * i && t.way(MCQ_N_WAYS - 1u) == 16u * i;
        }
        McqTallyWays over = t;
        McqLaneAccWays a;
        hs::acc_of(r, a);
        over.add(a);
        ok = ok && over.way(0) == 0u && over.way(1) == 1u;
        report("10-bit fields", 1, ok);
    }
    { /* the per-seat flush: nothing from a clean wave, one atomic per word that is not zero, clear afterwards */
        const uint32_t tasks = 5;
        std::vector<uint64_t> recs((size_t)tasks * hs::kWave * hs::kRec);
        for (size_t i = 0; i < (size_t)tasks * hs::kWave; i++) legal(2, &recs[i * hs::kRec]);
        uint64_t row[32] = {}, want[32] = {};
        hs::fold<McqLaneAccSeats>(recs.data(), (uint64_t)tasks * hs::kWave, want);
        McqTallySeats st[hs::kWave];
        for (uint32_t l = 0; l < hs::kWave; l++) st[l].clear();
        bool ok = hs::flush_seats(st, row) == 0u && hs::wave_seats(st, recs.data(), tasks);
        uint32_t nonzero = 0;
        for (uint32_t w = 1; w < 32; w++) nonzero += want[w] ? 1u : 0u;
        ok = ok && hs::flush_seats(st, row) == nonzero && memcmp(row, want, sizeof row) == 0 && hs::flush_seats(st, row) == 0u;
        for (uint32_t l = 0; l < hs::kWave; l++) ok = ok && hs::is_clear(st[l]);
        report("flush", 2, ok);
    }
    if (failed) printf("FAILED: %u of %u\n", failed, cases);
    else printf("ok: %u\n", cases);
    return failed ? 1 : 0;
}
