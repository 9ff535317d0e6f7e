#!/usr/bin/env python3
"""Timing of mcq_exact_batch_hero_range (every hand of a hero range from one enumeration) beside the other way to the same
rows: ONE batched mcq_exact_batch_ext call with one record per allowed hero hand.

    python tools/hero_range_probe.py                     call times (host clock around calls that end in a synchronise),
                                                         the two ways alternating, after a warm-up of every shape
    rocprofv3 --kernel-trace --output-format csv -d DIR -o hero -- python tools/hero_range_probe.py --trace
    python tools/hero_range_probe.py --kernels DIR/.../hero_kernel_trace.csv
                                                         kernel times from that trace (a run of its own: tracing slows the host)

Both ways are checked to give the same rows before anything is timed.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("flop, any vs any", None, None, ["2D", "9H", "JS"]),
          ("flop, top 25% vs top 25%", 0.25, 0.25, ["2D", "9H", "JS"]),
          ("turn, any vs any", None, None, ["2D", "9H", "JS", "5C"])]
ROUNDS, TRACE_ROUNDS = 20, 5
OLD_KERNEL, NEW_KERNEL = "mcq_exact_ext_kernel", "mcq_exact_hero_kernel"


def in_range(bits, a, b):
    """Is the class of two cards in a 169-bit set?  (include/mcq.h: suited 13 * min + max, off-suit 13 * max + min, pair 14 * rank)"""
    ra, rb = a >> 2, b >> 2
    lo, hi = min(ra, rb), max(ra, rb)
    i = 14 * ra if ra == rb else 13 * lo + hi if (a & 3) == (b & 3) else 13 * hi + lo
    return (int(bits[i >> 5]) >> (i & 31)) & 1


def shapes():
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    out = []
    for name, hero, opp, table in SHAPES:
        t = [npa.card_id(c) for c in table]
        hb = _opponent_range_bits(1 if hero is None else hero)
        ob = _opponent_range_bits(1 if opp is None else opp)
        q = _lib.pack_query_one([0, 0], t, 2, 1)
        x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES if hb is None else hb, opp_range=ob)
        deck = [c for c in range(52) if c not in t]
        hands = [(a, b) for b in deck for a in deck if a < b and (hb is None or in_range(hb, a, b))]
        hq = np.concatenate([_lib.pack_query_one(list(h), t, 2, 1) for h in hands])
        hx = _lib.pack_query_ext(len(hands), opp_range=ob)
        out.append((name, q, x, hq, hx, [_lib.hand_index(*h) for h in hands]))
    return out


def run(trace):
    import neuron_poker_amd as npa
    eng = npa.Engine(0)
    rounds = TRACE_ROUNDS if trace else ROUNDS
    for name, q, x, hq, hx, idx in shapes():
        new = lambda: eng.exact_hero_range(q, x, "reference")  # noqa: E731
        old = lambda: eng.exact_ext(hq, hx, "reference")       # noqa: E731
        rows, _ = new()                                         # warm-up of this shape, and the check
        _, one = old()
        assert np.array_equal(rows[0][idx].view(np.uint64), one.view(np.uint64)), name
        assert int((rows[0]["runs"] != 0).sum()) == len(idx)
        t_new, t_old = [], []
        for _ in range(rounds):                                 # alternating: what else runs on the host hits both alike
            t0 = time.perf_counter()
            new()
            t1 = time.perf_counter()
            old()
            t2 = time.perf_counter()
            t_new.append(t1 - t0)
            t_old.append(t2 - t1)
        if trace:
            print("%s: %d hero hands, %d dispatches of each way" % (name, len(idx), 1 + rounds), flush=True)
            continue
        mn, mo = np.median(t_new) * 1e3, np.median(t_old) * 1e3
        print("%-26s %4d hero hands  call: one record per hand %9.3f ms (min %8.3f)  hero range %8.3f ms (min %7.3f)  ratio %6.1fx"
              % (name, len(idx), mo, min(t_old) * 1e3, mn, min(t_new) * 1e3, mo / mn), flush=True)
    eng.close()


def kernels(path):
    """The trace holds, per shape and in this order, 1 + TRACE_ROUNDS dispatches of each way; the first of each is the warm-up."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = {OLD_KERNEL: [], NEW_KERNEL: []}
    for r in rows:
        for k in dur:
            if k in r["Kernel_Name"]:
                dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    n = 1 + TRACE_ROUNDS
    assert len(dur[OLD_KERNEL]) == len(dur[NEW_KERNEL]) == n * len(SHAPES), (len(dur[OLD_KERNEL]), len(dur[NEW_KERNEL]))
    for i, (name, _, _, _) in enumerate(SHAPES):
        o, w = np.median(dur[OLD_KERNEL][i * n + 1:(i + 1) * n]), np.median(dur[NEW_KERNEL][i * n + 1:(i + 1) * n])
        print("%-26s kernel: one record per hand %9.3f ms  hero range %8.3f ms  ratio %6.1fx" % (name, o, w, o / w))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true", help="few rounds, no timing: the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernels", metavar="CSV", help="read kernel times from a kernel trace of a --trace run")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels)
    else:
        run(a.trace)
