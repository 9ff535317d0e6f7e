#!/usr/bin/env python3
"""Timing of mcq_eval_batch_ranges (a weighted range per seat, the joint law) beside mcq_eval_batch_ext_seats on the same
records with the same class range (the reference's law, hero's hand known) -- with --baseline-lib, the latter from ANOTHER
build of the library (the parent commit's), loaded next to this one.

    python tools/ranges_timing.py [--baseline-lib PATH] [--out profiles/r18_ranges.txt]

2048 flop records x 20 000 runs: random flops, the hero one-hot on a random hand, every opponent on the top quarter of the
classes as ONE shared 0/1 table; six seats and a three-seat line.  The ten-seat line seats nine opponents on EVERY class:
nine disjoint hands out of the top quarter (292 hands crowded on the high cards) are not found within the trial bound, and
the entry refuses such a record.  Kernel time is the evaluation kernel's
own (the timestamp events of mcq_set_kernel_timing), the median of ROUNDS calls after a warm-up; evaluations = seven-card
hands ranked = records x seats x runs.  The two laws differ -- here every trial deals ALL seats and one collision abandons
it, there every opponent is re-drawn alone from its candidate list -- so trials per iteration stand next to the ratio."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, RUNS, ROUNDS, GEN_SEED = 2048, 20000, 5, 20240613
SHAPES = ((6, 0.25), (3, 0.25), (10, 1.0))   # seats, the opponents' top fraction of the classes


class Baseline:
    """mcq_eval_batch_ext_seats of another build of the library, through its C ABI alone."""

    def __init__(self, path):
        L = self.lib = C.CDLL(os.path.abspath(path))
        vp, u64 = C.c_void_p, C.c_uint64
        L.mcq_create.restype = vp
        L.mcq_create.argtypes = [C.c_int, C.c_int]
        L.mcq_destroy.argtypes = [vp]
        L.mcq_set_kernel_timing.argtypes = [vp, C.c_int]
        L.mcq_last_kernel_ms.argtypes = [vp]
        L.mcq_last_kernel_ms.restype = C.c_float
        L.mcq_eval_batch_ext_seats.argtypes = [vp, vp, vp, C.c_size_t, u64, u64, C.c_int, vp]
        self.ctx = L.mcq_create(0, 0)
        assert self.ctx, "mcq_create of the baseline library failed"
        assert L.mcq_set_kernel_timing(self.ctx, 1) == 0

    def ext_seats(self, q, x, seed):
        out = np.zeros((len(q), 32), np.uint64)
        rc = self.lib.mcq_eval_batch_ext_seats(self.ctx, q.ctypes.data, x.ctypes.data, len(q), seed, 0, 0, out.ctypes.data)
        assert rc == 0, rc
        return out, float(self.lib.mcq_last_kernel_ms(self.ctx))

    def close(self):
        self.lib.mcq_destroy(self.ctx)


def records(seats, top):
    """-> (queries, extension records of the class-range form, seat_table, tables)"""
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits, _seat_table
    g = np.random.default_rng(GEN_SEED)
    cards = np.array([g.permutation(52)[:5] for _ in range(N)], np.uint8)
    board = np.full((N, 5), 255, np.uint8)
    board[:, :3] = cards[:, 2:]
    q = _lib.pack_queries(cards[:, :2], board, seats, RUNS)
    x = _lib.pack_query_ext(N, opp_range=_opponent_range_bits(top))
    tables = np.zeros((1 + N, 1326), np.uint16)
    tables[0] = _seat_table(top, "opponents")
    for i in range(N):
        tables[1 + i, _lib.hand_index(cards[i, 0], cards[i, 1])] = 1
    st = np.zeros((N, 10), np.uint32)
    st[:, 0] = 1 + np.arange(N)
    return q, x, st, tables


def median(f):
    f()   # warm-up: buffers, clocks
    return float(np.median([f() for _ in range(ROUNDS)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--out", default=os.path.join("profiles", "r18_ranges.txt"))
    a = ap.parse_args()
    import neuron_poker_amd as npa
    eng = npa.Engine(0, kernel_times=True)
    base = Baseline(a.baseline_lib) if a.baseline_lib else None
    lines = ["# %d flop records x %d runs; hero one-hot, the opponents on one shared 0/1 table of the top classes" % (N, RUNS),
             "# ranges = mcq_eval_batch_ranges (joint law); ext_seats = mcq_eval_batch_ext_seats (class range, reference law)%s"
             % (" of the baseline library" if base else " of this library")]
    for seats, top in SHAPES:
        q, x, st, tables = records(seats, top)
        evals = float(N) * seats * RUNS
        trials = [0.0]

        def ranges():
            rows = eng.eval_batch_ranges(q, st, tables, 1)
            trials[0] = float(rows["passes"].sum()) / float(rows["runs"].sum())
            return float(eng.last_kernel_ms)
        ext_trials = [0.0]

        def ext():
            if base:
                rows, ms = base.ext_seats(q, x, 1)
                ext_trials[0] = float(rows[:, 1].sum()) / float(rows[:, 0].sum())
                return ms
            rows = eng.eval_batch_ext_seats(q, x, 1)
            ext_trials[0] = float(rows["passes"].sum()) / float(rows["runs"].sum())
            return float(eng.last_kernel_ms)
        ms_r, ms_e = median(ranges), median(ext)
        lines.append("%2d seats, top %3.0f %%: ranges %9.3f ms  %.3e evaluations/s  passes/runs %.3f (whole trials) | ext_seats %9.3f ms  "
                     "%.3e evaluations/s  passes/runs %.3f (opponent trials) | ranges / ext_seats %.2f"
                     % (seats, 100 * top, ms_r, evals / (ms_r * 1e-3), trials[0], ms_e, evals / (ms_e * 1e-3), ext_trials[0], ms_r / ms_e))
        print(lines[-1], flush=True)
    if base:
        base.close()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
