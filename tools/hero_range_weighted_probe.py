#!/usr/bin/env python3
"""Timing of mcq_exact_batch_hero_range_weighted (a weight per hand, every weight 1 here) beside mcq_exact_batch_hero_range
under the uniform law on the same records -- and, with --baseline-lib, beside the same unweighted entry of ANOTHER build of
the library (the parent commit's), loaded next to this one: what the weights cost, and that the unweighted entry did not
get slower.

    python tools/hero_range_weighted_probe.py [--baseline-lib PATH]
                                call times (host clock around calls that end in a synchronise), medians of alternating
                                rounds after a warm-up of every shape
    rocprofv3 --kernel-trace --output-format csv -d DIR -o wprobe -- python tools/hero_range_weighted_probe.py --trace [--baseline-lib PATH]
    python tools/hero_range_weighted_probe.py --kernels DIR/.../wprobe_kernel_trace.csv [--baseline-lib PATH]
                                kernel times from that trace (a run of its own: tracing slows the host)

The three ways are checked to give the same rows before anything is timed.
"""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("flop, any vs any", None, None, ["2D", "9H", "JS"]),
          ("flop, top 25% vs top 25%", 0.25, 0.25, ["2D", "9H", "JS"]),
          ("turn, any vs any", None, None, ["2D", "9H", "JS", "5C"])]
ROUNDS, TRACE_ROUNDS = 20, 5
PLAIN_KERNEL, WEIGHTED_KERNEL = "mcq_exact_hero_kernel", "mcq_exact_hero_w_kernel"


class Baseline:
    """mcq_exact_batch_hero_range of another build of the library, through its C ABI alone."""

    def __init__(self, path):
        self.lib = C.CDLL(os.path.abspath(path))
        self.lib.mcq_create.restype = C.c_void_p
        self.lib.mcq_create.argtypes = [C.c_int, C.c_uint]
        self.lib.mcq_destroy.argtypes = [C.c_void_p]
        vp = C.c_void_p
        self.lib.mcq_exact_batch_hero_range.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, vp]
        self.ctx = self.lib.mcq_create(0, 0)
        assert self.ctx, "mcq_create of the baseline library failed"

    def hero_range(self, q, x, rows, agg):
        rc = self.lib.mcq_exact_batch_hero_range(self.ctx, q.ctypes.data, x.ctypes.data, len(q), 1, rows.ctypes.data, agg.ctypes.data)
        assert rc == 0, rc
        return rows

    def close(self):
        self.lib.mcq_destroy(self.ctx)


def shapes():
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    out = []
    for name, hero, opp, table in SHAPES:
        hb = _opponent_range_bits(1 if hero is None else hero)
        ob = _opponent_range_bits(1 if opp is None else opp)
        q = _lib.pack_query_one([0, 0], [npa.card_id(c) for c in table], 2, 1)
        x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES if hb is None else hb, opp_range=ob)
        out.append((name, q, x))
    return out


def run(trace, baseline_lib):
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    eng = npa.Engine(0)
    base = Baseline(baseline_lib) if baseline_lib else None
    ones = np.ones((1, _lib.HAND_ROWS), np.uint16)
    b_rows, b_agg = np.zeros((1, _lib.HAND_ROWS), _lib.RESULT_DTYPE), np.zeros(1, _lib.EXACT_PROB_DTYPE)
    rounds = TRACE_ROUNDS if trace else ROUNDS
    for name, q, x in shapes():
        ways = [("weighted", lambda: eng.exact_hero_range_weighted(q, x, ones)[0]),
                ("unweighted", lambda: eng.exact_hero_range(q, x, "uniform")[0])]
        if base:
            ways.append(("unweighted, baseline library", lambda: base.hero_range(q, x, b_rows, b_agg)))
        first = [f().tobytes() for _, f in ways]                    # warm-up of this shape, and the check
        assert all(r == first[0] for r in first), name
        times = [[] for _ in ways]
        for _ in range(rounds):                                     # alternating: what else runs on the host hits all alike
            for t, (_, f) in zip(times, ways):
                t0 = time.perf_counter()
                f()
                t.append(time.perf_counter() - t0)
        hands = int((np.frombuffer(first[0], _lib.RESULT_DTYPE)["runs"] != 0).sum())
        if trace:
            print("%s: %d hero hands, %d dispatches of each way" % (name, hands, 1 + rounds), flush=True)
            continue
        med = [np.median(t) * 1e3 for t in times]
        print("%-26s %4d hero hands  call:" % (name, hands) +
              "".join("  %s %8.3f ms (min %7.3f)" % (w[0], m, min(t) * 1e3) for w, m, t in zip(ways, med, times)) +
              "  weighted / unweighted %5.2fx" % (med[0] / med[1]) +
              ("  unweighted / baseline %5.2fx" % (med[1] / med[2]) if base else ""), flush=True)
    eng.close()
    if base:
        base.close()


def kernels(path, baseline):
    """The trace holds, per shape and in this order, 1 + TRACE_ROUNDS rounds of one dispatch per way; the first round is
    the warm-up.  The unweighted kernel of this library and of the baseline carry the same name: they alternate."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {PLAIN_KERNEL: [], WEIGHTED_KERNEL: []}
    for r in rows:
        for k in dur:
            if k in r["Kernel_Name"]:                               # (neither name is part of the other)
                dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    n, per = 1 + TRACE_ROUNDS, 2 if baseline else 1
    assert len(dur[WEIGHTED_KERNEL]) == n * len(SHAPES) and len(dur[PLAIN_KERNEL]) == per * n * len(SHAPES), \
        (len(dur[WEIGHTED_KERNEL]), len(dur[PLAIN_KERNEL]))
    for i, (name, _, _, _) in enumerate(SHAPES):
        w = np.median(dur[WEIGHTED_KERNEL][i * n + 1:(i + 1) * n])
        plain = dur[PLAIN_KERNEL][per * (i * n + 1):per * (i + 1) * n]
        p = np.median(plain[0::per])
        line = "%-26s kernel: weighted %8.3f ms  unweighted %8.3f ms  weighted / unweighted %5.2fx" % (name, w, p, w / p)
        if baseline:
            b = np.median(plain[1::per])
            line += "  unweighted, baseline library %8.3f ms  unweighted / baseline %5.2fx" % (b, p / b)
        print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", metavar="SO", help="another build of libmcq_hip.so whose unweighted entry is timed too")
    ap.add_argument("--trace", action="store_true", help="few rounds, no timing: the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernels", metavar="CSV", help="read kernel times from a kernel trace of a --trace run")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels, bool(a.baseline_lib))
    else:
        run(a.trace, a.baseline_lib)
