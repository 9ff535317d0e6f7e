#!/usr/bin/env python3
"""Timing of mcq_exact_batch_hero_range_preflop_weighted (weighted hands before the flop) with every weight 1 beside
mcq_exact_batch_hero_range_preflop under the uniform law, which then gives the same rows: what the weight tables, the lists
made from them and the 64-bit sums cost or save against the class bits.

    timeout -k 10 240 python tools/hero_preflop_weighted_probe.py --cases a [--baseline-lib PATH]
    timeout -k 10 60 python tools/hero_preflop_weighted_probe.py --cases b [--baseline-lib PATH]
    timeout -k 10 60 python tools/hero_preflop_weighted_probe.py --cases c [--baseline-lib PATH]
                                call times (host clock around calls that end in a synchronise), the entries alternating,
                                after a warm-up of the shape; per entry the median and the spread (min .. max) of the
                                rounds.  One case per process, each under a time limit of its own and chained with &&:
                                nothing more is started on a GPU after a step that faulted or hung.
                                --baseline-lib: the unweighted entry of ANOTHER build of the library (the parent
                                commit's), loaded next to this one, is timed too: that the unweighted entry did not
                                get slower
    timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d DIR -o prew -- python tools/hero_preflop_weighted_probe.py --trace
    python tools/hero_preflop_weighted_probe.py --kernels DIR/.../prew_kernel_trace.csv
                                the launches of case (a), one call per entry: their number, the longest one and their
                                sum (a run of its own: tracing slows the host; --kernels reads the file, no GPU)
    timeout -k 10 540 python tools/hero_preflop_weighted_probe.py --ab PARENT_SO COPY_SO
                                all FOUR hero-range entries, postflop and preflop, the unweighted ones under both
                                laws, of this build beside the parent commit's build and a second copy of it (see
                                ab()): exit status 1 unless every ratio lies inside the widened interval

The rows and aggregates of the two entries are checked to be equal byte for byte before anything is timed.
"""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# key, name, hero range, opponent range, timed rounds
SHAPES = [("a", "any vs any", None, None, 3),
          ("b", "top 25% vs top 25%", 0.25, 0.25, 5),
          ("c", "{AA, AKs} vs top 10%", {"AA", "AKS"}, 0.10, 15)]
KERNELS = [("unweighted", "mcq_exact_hero_pre_kernel"), ("weighted", "mcq_exact_hero_pre_w_kernel")]


class Baseline:
    """The four hero-range entries of another build of the library, through its C ABI alone."""

    def __init__(self, path):
        self.lib = C.CDLL(os.path.abspath(path))
        self.lib.mcq_create.restype = C.c_void_p
        self.lib.mcq_create.argtypes = [C.c_int, C.c_uint]
        self.lib.mcq_destroy.argtypes = [C.c_void_p]
        vp = C.c_void_p
        for street in ("", "_preflop"):
            getattr(self.lib, "mcq_exact_batch_hero_range" + street).argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, vp]
            getattr(self.lib, "mcq_exact_batch_hero_range%s_weighted" % street).argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
        self.ctx = self.lib.mcq_create(0, 0)
        assert self.ctx, "mcq_create of the baseline library failed"

    def call(self, entry, q, x, rows, agg, opp_w=None, law=1):
        """mcq_exact_batch_<entry>: under `law` (0 reference, 1 uniform), or (a ..._weighted entry) with the opponent's table
        opp_w alone"""
        mid = (law,) if opp_w is None else (opp_w.ctypes.data, None)
        rc = getattr(self.lib, "mcq_exact_batch_" + entry)(self.ctx, q.ctypes.data, x.ctypes.data, len(q), *mid, rows.ctypes.data,
                                                           agg.ctypes.data)
        assert rc == 0, rc
        return rows, agg

    def preflop(self, q, x, rows, agg):
        return self.call("hero_range_preflop", q, x, rows, agg)

    def close(self):
        self.lib.mcq_destroy(self.ctx)


def shapes(keys):
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    out = []
    for key, name, hero, opp, rounds in SHAPES:
        if key not in keys:
            continue
        hb = _opponent_range_bits(1 if hero is None else hero)
        ob = _opponent_range_bits(1 if opp is None else opp)
        q = _lib.pack_query_one([0, 0], [], 2, 1)
        x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES if hb is None else hb, opp_range=ob)
        out.append((key, name, q, x, rounds))
    return out


def run(keys, baseline_lib):
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    eng = npa.Engine(0)
    base = Baseline(baseline_lib) if baseline_lib else None
    ones = np.ones((1, _lib.HAND_ROWS), np.uint16)
    b_rows, b_agg = np.zeros((1, _lib.HAND_ROWS), _lib.RESULT_DTYPE), np.zeros(1, _lib.EXACT_PROB_DTYPE)
    for key, name, q, x, rounds in shapes(keys):
        ways = [("weighted, every weight 1", lambda: eng.exact_hero_range_preflop_weighted(q, x, ones)),
                ("unweighted, uniform law", lambda: eng.exact_hero_range_preflop(q, x, "uniform"))]
        if base:
            ways.append(("unweighted, baseline library", lambda: base.preflop(q, x, b_rows, b_agg)))
        first = [f() for _, f in ways]                                     # warm-up of this shape, and the check
        assert all(r.tobytes() == first[0][0].tobytes() and a.tobytes() == first[0][1].tobytes() for r, a in first), name
        n_hands = int((first[0][0][0]["runs"] != 0).sum())
        times = [[] for _ in ways]
        for _ in range(rounds):                                            # alternating: what else runs on the host hits all alike
            for t, (_, f) in zip(times, ways):
                t0 = time.perf_counter()
                f()
                t.append((time.perf_counter() - t0) * 1e3)
        med = [np.median(t) for t in times]
        print("(%s) %-22s %4d hero hands, %d rounds " % (key, name, n_hands, rounds) +
              "".join("  %s %9.2f ms (%.2f .. %.2f)" % (w[0], m, min(t), max(t)) for w, m, t in zip(ways, med, times)) +
              "  weighted / unweighted %5.3f" % (med[0] / med[1]) +
              ("  unweighted / baseline %5.3f" % (med[1] / med[2]) if base else ""), flush=True)
    eng.close()
    if base:
        base.close()


# --ab: name, table cards, hero range, opponent range, timed rounds per call order -- the shapes of tools/hero_range_probe.py
# and tools/hero_range_weighted_probe.py, then SHAPES above
AB_SHAPES = [("flop, any vs any", ["2D", "9H", "JS"], None, None, 10),
             ("flop, top 25% vs top 25%", ["2D", "9H", "JS"], 0.25, 0.25, 10),
             ("turn, any vs any", ["2D", "9H", "JS", "5C"], None, None, 10)] + \
            [("preflop, " + name, [], hero, opp, rounds // 3) for _, name, hero, opp, rounds in SHAPES]
AB_PASSES = 4


def ab_cases(ab_shapes):
    """The cases of tools/ab_common.py's loop for the four hero-range entries on ab_shapes (entries as AB_SHAPES): an
    unweighted entry is timed under the reference's law, its default, and under the uniform one -- the walks are separate
    copies of the loop per law, or read the law per candidate."""
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    ones = np.ones((1, _lib.HAND_ROWS), np.uint16)
    out = [(np.zeros((1, _lib.HAND_ROWS), _lib.RESULT_DTYPE), np.zeros(1, _lib.EXACT_PROB_DTYPE)) for _ in range(3)]
    cases = []
    for name, table, hero, opp, rounds in ab_shapes:
        hb, ob = _opponent_range_bits(1 if hero is None else hero), _opponent_range_bits(1 if opp is None else opp)
        q = _lib.pack_query_one([0, 0], [npa.card_id(c) for c in table], 2, 1)
        x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES if hb is None else hb, opp_range=ob)
        street = "hero_range" + ("" if table else "_preflop")
        for entry, label, w, law in ((street, name + ", reference law", None, 0), (street, name, None, 1),
                                     (street + "_weighted", name, ones, 1)):
            cases.append(((entry, label), rounds,
                          lambda b, slot, entry=entry, q=q, x=x, w=w, law=law: b.call(entry, q, x, out[slot][0], out[slot][1], w, law)))
    return cases


def ab(parent_so, copy_so):
    """All four entries of this build beside the parent commit's build and a second copy of it, by the loop and the rule of
    tools/ab_common.py (the two long preflop shapes get ONE timed call per order and pass, so their "median" is that call:
    a call of seconds, whose rounds differ by under 0.2 %, profiles/hero_preflop_weighted_probe.txt).  "faster" fails like
    "OUTSIDE": the rule is inside, and a loop that got faster on one shape has changed and may be slower on another."""
    import ab_common
    from neuron_poker_amd import _lib
    _lib.load_library()
    return ab_common.ab(Baseline, (_lib.library_path(), parent_so, copy_so), ab_cases(AB_SHAPES), AB_PASSES, faster_fails=True)


def trace():
    """Case (a) alone, one call per entry and no warm-up call of it: every launch of a kernel belongs to that call."""
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    eng = npa.Engine(0)
    (_, name, q, x, _), = shapes("a")
    rows, _ = eng.exact_hero_range_preflop(q, x, "uniform")
    print("%s, unweighted: %d rows with weight" % (name, int((rows[0]["runs"] != 0).sum())), flush=True)
    rows, _ = eng.exact_hero_range_preflop_weighted(q, x, np.ones((1, _lib.HAND_ROWS), np.uint16))
    print("%s, weighted: %d rows with weight" % (name, int((rows[0]["runs"] != 0).sum())), flush=True)
    eng.close()


def kernels(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for label, kernel in KERNELS:
        mine = sorted((r for r in rows if kernel in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine]
        assert d, kernel
        print("(a) any vs any, %-10s %d launches: longest %.2f ms, median %.2f ms, sum %.2f ms" % (label, len(d), max(d), np.median(d), sum(d)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc", help="which of the cases a, b, c to time (one per process under a time limit, see above)")
    ap.add_argument("--baseline-lib", metavar="SO", help="another build of libmcq_hip.so whose unweighted entry is timed too")
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_SO", "COPY_SO"),
                    help="all four hero-range entries of this build beside the parent's build and a second copy of it, both call orders")
    ap.add_argument("--trace", action="store_true", help="case (a) once per entry, no timing: the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernels", metavar="CSV", help="read the launches' times from a kernel trace of a --trace run")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels)
    elif a.ab:
        sys.exit(0 if ab(*a.ab) else 1)
    elif a.trace:
        trace()
    else:
        run(a.cases, a.baseline_lib)
