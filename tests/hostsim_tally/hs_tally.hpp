// hs_tally.hpp -- TEST HARNESS ONLY: a wave of 64 lanes for the lane states and the lanes -> row step of
// neuron_poker_amd/csrc/mcq_tally.hpp, shared by hs_tally.cpp (the library the tests load) and hs_main.cpp (the program
// the tests run under the host sanitizers).
//
// The stand-in for the wave reduction works in two passes.  Every lane runs the same sequence of reductions, so in the
// first pass each lane's step runs on a copy of its state with a functor that records the k-th argument and returns 0;
// the k-th totals over the 64 lanes are formed (32-bit, as the device adds); in the second pass the step runs on the
// state itself and the functor hands the totals back in the same order.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace hs {
constexpr uint32_t kWave = 64, kRec = 12; /* an accumulator travels as kRec 64-bit words, see acc_of */

struct Tape {
    std::vector<uint32_t> v; /* pass one: this lane's arguments; pass two: the wave's totals */
    size_t at = 0;
    bool play = false;
};
struct TapeSum {
    Tape *t;
    uint32_t operator()(uint32_t x) const {
        if (t->play) return t->v.at(t->at++);
        t->v.push_back(x);
        return 0u;
    }
};
/* step(state, lane, sum) -> the lane's 64-bit word.  -> false if the lanes did not issue the same number of reductions */
template <class State, class Step> bool wave_step(State *st, Step step, uint64_t *out) {
    Tape rec[kWave];
    for (uint32_t l = 0; l < kWave; l++) {
        State copy = st[l];
        step(copy, l, TapeSum{&rec[l]});
    }
    Tape tot;
    tot.play = true;
    tot.v.assign(rec[0].v.size(), 0u);
    for (uint32_t l = 0; l < kWave; l++) {
        if (rec[l].v.size() != tot.v.size()) return false;
        for (size_t k = 0; k < tot.v.size(); k++) tot.v[k] += rec[l].v[k];
    }
    for (uint32_t l = 0; l < kWave; l++) {
        tot.at = 0;
        const uint64_t w = step(st[l], l, TapeSum{&tot});
        if (out) out[l] = w;
        if (tot.at != tot.v.size()) return false;
    }
    return true;
}

/* records: plain {types, tie, passes}, ways {types, passes, ways}, seats {passes, seat[0..9]} */
inline void acc_of(const uint64_t *r, McqLaneAcc &a) { a.types = r[0]; a.tie = (uint32_t)r[1]; a.passes = (uint32_t)r[2]; }
inline void acc_of(const uint64_t *r, McqLaneAccWays &a) { a.types = r[0]; a.passes = (uint32_t)r[1]; a.ways = r[2]; }
inline void acc_of(const uint64_t *r, McqLaneAccSeats &a) {
    a.passes = (uint32_t)r[0];
    for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) a.seat[s] = (uint32_t)r[1 + s];
}

/* rows += the fold of n records */
template <class Acc> void fold(const uint64_t *recs, uint64_t n, uint64_t *row) {
    for (uint64_t i = 0; i < n; i++) {
        Acc a;
        acc_of(recs + i * kRec, a);
        mcq_tally_fold(a, row);
    }
}

/* recs[task][lane][kRec]: clear, add n_tasks tasks in every lane -> the 64 lane states */
template <class Tally> void add_tasks(Tally *st, const uint64_t *recs, uint32_t n_tasks) {
    for (uint32_t l = 0; l < kWave; l++) st[l].clear();
    for (uint32_t t = 0; t < n_tasks; t++)
        for (uint32_t l = 0; l < kWave; l++) {
            typename Tally::Acc a;
            acc_of(recs + ((size_t)t * kWave + l) * kRec, a);
            st[l].add(a);
        }
}
/* ... -> the word every lane ends up holding.  packed: row_words (two counters per reduction), else row_value */
template <class Tally> bool wave_words(const uint64_t *recs, uint32_t n_tasks, bool packed, uint64_t *words) {
    Tally st[kWave];
    add_tasks(st, recs, n_tasks);
    return wave_step(st, [&](Tally &t, uint32_t lane, TapeSum sum) { return packed ? t.row_words(lane, sum) : t.row_value(lane, sum); }, words);
}
/* the per-seat kind: a wave step per task, the lane's register afterwards */
inline bool wave_seats(McqTallySeats *st, const uint64_t *recs, uint32_t n_tasks) {
    for (uint32_t l = 0; l < kWave; l++) st[l].clear();
    for (uint32_t t = 0; t < n_tasks; t++) {
        const uint64_t *task = recs + (size_t)t * kWave * kRec;
        const bool ok = wave_step(st, [&](McqTallySeats &s, uint32_t lane, TapeSum sum) {
            McqLaneAccSeats a;
            acc_of(task + (size_t)lane * kRec, a);
            s.add(a, lane, sum);
            return s.mine;
        }, nullptr);
        if (!ok) return false;
    }
    return true;
}

/* the stand-in for the atomic: adds and counts */
struct CountingAdd {
    uint32_t *n;
    void operator()(uint64_t *word, uint64_t v) const {
        *word += v;
        ++*n;
    }
};
inline bool codes_clear(const McqTallyCodes &t) {
    for (uint32_t c = 0; c < MCQ_N_CODES; c++)
        if (t.code[c]) return false;
    return true;
}
inline bool is_clear(const McqTally &t) { return codes_clear(t) && !t.tie && !t.passes && !t.dirty; }
inline bool is_clear(const McqTallyWays &t) { return codes_clear(t) && !t.passes && !t.way3[0] && !t.way3[1] && !t.way3[2] && !t.n_add && !t.dirty; }
inline bool is_clear(const McqTallySeats &s) { return s.mine == 0 && !s.dirty; }
/* the per-seat flush of a wave whose lanes hold their words: atomics issued */
inline uint32_t flush_seats(McqTallySeats *st, uint64_t *row) {
    uint32_t n = 0;
    for (uint32_t l = 0; l < kWave; l++) st[l].flush(row, l, CountingAdd{&n});
    return n;
}
}  // namespace hs
