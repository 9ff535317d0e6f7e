// hs_tally.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Host build of the wave tallies (neuron_poker_amd/csrc/mcq_tally.hpp): the fold of an accumulator into a row, and the
// real lane states and lanes -> row step run for a simulated wave of 64 lanes (hs_tally.hpp), so that
// tests/test_tally_host.py can hold them to an unpacking of its own where no GPU exists.
// kind: 0 plain (McqLaneAcc), 1 split-pot (McqLaneAccWays), 2 per-seat (McqLaneAccSeats).
#include "hs_tally.hpp"

extern "C" {

// words and lanes of the three row kinds, the two task limits, codes, ways, seats
void hs_tally_consts(uint32_t *out) {
    const uint32_t v[] = {McqTally::kWords, McqTally::kLanes, McqTallyWays::kWords, McqTallyWays::kLanes, McqTallySeats::kWords,
                          McqTallySeats::kLanes, MCQ_WAYS_TALLY_TASKS, MCQ_DIRECT_TASKS_LIMIT, MCQ_N_CODES, MCQ_N_WAYS, MCQ_MAX_SEATS};
    memcpy(out, v, sizeof v);
}

// row (32 words, the caller's) += the fold of n records
int hs_tally_fold(uint32_t kind, const uint64_t *recs, uint64_t n, uint64_t *row) {
    if (kind == 0) hs::fold<McqLaneAcc>(recs, n, row);
    else if (kind == 1) hs::fold<McqLaneAccWays>(recs, n, row);
    else if (kind == 2) hs::fold<McqLaneAccSeats>(recs, n, row);
    else return MCQ_EINVAL;
    return MCQ_OK;
}

// recs[n_tasks][64][12] added to a cleared wave -> words[64]: what every lane holds after row_value (packed = 0) or
// row_words (packed != 0); the per-seat kind: after an add per task
int hs_tally_wave(uint32_t kind, uint32_t packed, const uint64_t *recs, uint32_t n_tasks, uint64_t *words) {
    if (kind == 0) return hs::wave_words<McqTally>(recs, n_tasks, packed != 0, words) ? MCQ_OK : MCQ_EINVAL;
    if (kind == 1) return hs::wave_words<McqTallyWays>(recs, n_tasks, packed != 0, words) ? MCQ_OK : MCQ_EINVAL;
    if (kind != 2) return MCQ_EINVAL;
    McqTallySeats st[hs::kWave];
    if (!hs::wave_seats(st, recs, n_tasks)) return MCQ_EINVAL;
    for (uint32_t l = 0; l < hs::kWave; l++) words[l] = st[l].mine;
    return MCQ_OK;
}

// the split-pot lane state after n_tasks tasks of one record each (recs[n_tasks][12]), without a flush:
// out = way3[3], n_add, full(), way(0..8)
void hs_tally_ways_state(const uint64_t *recs, uint32_t n_tasks, uint32_t *out) {
    McqTallyWays t;
    t.clear();
    for (uint32_t i = 0; i < n_tasks; i++) {
        McqLaneAccWays a;
        hs::acc_of(recs + (size_t)i * hs::kRec, a);
        t.add(a);
    }
    out[0] = t.way3[0];
    out[1] = t.way3[1];
    out[2] = t.way3[2];
    out[3] = t.n_add;
    out[4] = t.full() ? 1u : 0u;
    for (uint32_t k = 0; k < MCQ_N_WAYS; k++) out[5 + k] = t.way(k);
}

// The per-seat flush (the one flush the header holds; the other kinds' is a wrapper in mcq_kernels.hip around row_value):
// row (32 words) += the wave's words through a counting stand-in for the atomic.
// out = atomics issued by the flush of a clean wave, by the flush after the tasks, by a second flush; every lane clear afterwards
int hs_tally_seats_flush(const uint64_t *recs, uint32_t n_tasks, uint64_t *row, uint32_t *out) {
    McqTallySeats st[hs::kWave];
    for (uint32_t l = 0; l < hs::kWave; l++) st[l].clear();
    out[0] = hs::flush_seats(st, row);
    if (!hs::wave_seats(st, recs, n_tasks)) return MCQ_EINVAL;
    out[1] = hs::flush_seats(st, row);
    out[3] = 1u;
    for (uint32_t l = 0; l < hs::kWave; l++)
        if (!hs::is_clear(st[l])) out[3] = 0u;
    out[2] = hs::flush_seats(st, row);
    return MCQ_OK;
}

// the plain and split-pot states: 1 if, after the tasks, clear() leaves every lane as a freshly cleared one -- what the
// kernels' flush (a wrapper in mcq_kernels.hip: not dirty -> nothing; else row_value, one atomic per word that is not
// zero, clear()) leaves behind -- and the wave's row_value and row_words of such lanes are zero in every lane
int hs_tally_clear_is_clean(uint32_t kind, const uint64_t *recs, uint32_t n_tasks) {
    auto check = [&](auto tag) {
        typedef decltype(tag) Tally;
        Tally st[hs::kWave];
        hs::add_tasks(st, recs, n_tasks);
        for (uint32_t l = 0; l < hs::kWave; l++) {
            if (!st[l].dirty) return false;
            st[l].clear();
            if (!hs::is_clear(st[l])) return false;
        }
        for (int packed = 0; packed < 2; packed++) {
            uint64_t words[hs::kWave];
            const bool ok = hs::wave_step(st, [&](Tally &t, uint32_t lane, hs::TapeSum sum) {
                return packed ? t.row_words(lane, sum) : t.row_value(lane, sum);
            }, words);
            if (!ok) return false;
            for (uint32_t l = 0; l < hs::kWave; l++)
                if (words[l]) return false;
        }
        return true;
    };
    if (kind == 0) return check(McqTally()) ? 1 : 0;
    if (kind == 1) return check(McqTallyWays()) ? 1 : 0;
    return -1;
}
}
