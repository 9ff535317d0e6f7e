#!/usr/bin/env python3
"""Timing of mcq_exact_batch_hero_range_preflop (every hand of a hero range before the flop from one enumeration) beside
the only other way to the same rows: ONE batched mcq_exact_batch_ext call with one record per allowed hero hand.

    python tools/hero_preflop_probe.py [--cases abc]     call times (host clock around calls that end in a synchronise),
                                                         the two ways alternating, after a warm-up of every shape; per
                                                         way the median and the spread (min .. max) of the rounds
    rocprofv3 --kernel-trace --output-format csv -d DIR -o pre -- python tools/hero_preflop_probe.py --trace
    python tools/hero_preflop_probe.py --kernels DIR/.../pre_kernel_trace.csv
                                                         the launches of case (a), one call per law: their number, the
                                                         longest one and their sum (a run of its own: tracing slows the host)

Both ways are checked to give the same rows before anything is timed.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# key, name, hero range, opponent range, timed rounds
SHAPES = [("a", "any vs any", None, None, 3),
          ("b", "top 25% vs top 25%", 0.25, 0.25, 5),
          ("c", "{AA, AKs} vs top 10%", {"AA", "AKS"}, 0.10, 15)]
LAWS = ["reference", "uniform"]
NEW_KERNEL = "mcq_exact_hero_pre_kernel"


def in_range(bits, a, b):
    """Is the class of two cards in a 169-bit set?  (include/mcq.h: suited 13 * min + max, off-suit 13 * max + min, pair 14 * rank)"""
    ra, rb = a >> 2, b >> 2
    lo, hi = min(ra, rb), max(ra, rb)
    i = 14 * ra if ra == rb else 13 * lo + hi if (a & 3) == (b & 3) else 13 * hi + lo
    return (int(bits[i >> 5]) >> (i & 31)) & 1


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
        hands = [(a, b) for b in range(52) for a in range(b) if hb is None or in_range(hb, a, b)]
        hq = np.concatenate([_lib.pack_query_one(list(h), [], 2, 1) for h in hands])
        hx = _lib.pack_query_ext(len(hands), opp_range=ob)
        out.append((key, name, q, x, hq, hx, [_lib.hand_index(*h) for h in hands], rounds))
    return out


def run(keys):
    import neuron_poker_amd as npa
    eng = npa.Engine(0)
    for key, name, q, x, hq, hx, idx, rounds in shapes(keys):
        for law in LAWS:
            new = lambda: eng.exact_hero_range_preflop(q, x, law)  # noqa: E731
            old = lambda: eng.exact_ext(hq, hx, law)               # noqa: E731
            rows, _ = new()                                         # warm-up of this shape, and the check
            _, one = old()
            assert np.array_equal(rows[0][idx].view(np.uint64), one.view(np.uint64)), (name, law)
            assert int((rows[0]["runs"] != 0).sum()) == len(idx)
            t_new, t_old = [], []
            for _ in range(rounds):                                 # alternating: what else runs on the host hits both alike
                t0 = time.perf_counter()
                new()
                t1 = time.perf_counter()
                old()
                t2 = time.perf_counter()
                t_new.append((t1 - t0) * 1e3)
                t_old.append((t2 - t1) * 1e3)
            mn, mo = np.median(t_new), np.median(t_old)
            print("(%s) %-22s %-9s %4d hero hands, %d rounds  one record per hand %10.2f ms (%.2f .. %.2f)  "
                  "hero range %9.2f ms (%.2f .. %.2f)  ratio %5.2fx (worst round against best: %.2fx)"
                  % (key, name, law, len(idx), rounds, mo, min(t_old), max(t_old), mn, min(t_new), max(t_new), mo / mn,
                     min(t_old) / max(t_new)), flush=True)
    eng.close()


def trace():
    """Case (a) alone, one call per law and no warm-up call of it: every launch of the new kernel belongs to one of them."""
    import neuron_poker_amd as npa
    eng = npa.Engine(0)
    (_, name, q, x, _, _, idx, _), = shapes("a")
    for law in LAWS:
        rows, _ = eng.exact_hero_range_preflop(q, x, law)
        print("%s, %s: %d rows with weight" % (name, law, int((rows[0]["runs"] != 0).sum())), flush=True)
    eng.close()


def kernels(path):
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if NEW_KERNEL in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    assert dur and len(dur) % len(LAWS) == 0, len(dur)
    n = len(dur) // len(LAWS)
    for i, law in enumerate(LAWS):
        d = dur[i * n:(i + 1) * n]
        print("(a) any vs any, %-9s %d launches: longest %.2f ms, median %.2f ms, sum %.2f ms" % (law, n, max(d), np.median(d), sum(d)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc", help="which of the cases a, b, c to time")
    ap.add_argument("--trace", action="store_true", help="case (a) once per law, no timing: the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernels", metavar="CSV", help="read the launches' times from a kernel trace of a --trace run")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels)
    elif a.trace:
        trace()
    else:
        run(a.cases)
