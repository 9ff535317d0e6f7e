#!/usr/bin/env python3
"""Timing of mcq_exact_batch_ext (exact enumeration of extended queries, SURVEY 8f-3 x 8f-2) on the GPU box, beside
the plain enumeration of the same shapes (mcq_exact_batch) for comparison."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neuron_poker_amd as npa  # noqa: E402
from neuron_poker_amd import _lib  # noqa: E402
from neuron_poker_amd.montecarlo_hip import _opponent_range_bits  # noqa: E402

eng = npa.Engine(0)
ids = lambda cs: [npa.card_id(c) for c in cs]  # noqa: E731


def timed(f, reps=5):
    f()                                         # warm: code objects loaded, buffers grown
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


top25 = _opponent_range_bits(0.25)
cases = [("AhAd vs KsKc preflop", ["AH", "AD"], [], 2, [["KS", "KC"]], None),
         ("AhKh vs top-25% preflop", ["AH", "KH"], [], 2, [], top25),
         ("9c8c + known vs 2 x top-25% flop", ["9C", "8C"], ["7C", "6D", "2S"], 4, [["AS", "AD"]], top25)]
for name, hero, board, n, known, rng in cases:
    q = _lib.pack_query_one(ids(hero), ids(board), n, 1)
    e = _lib.pack_query_ext(1, known=[ids(h) for h in known], opp_range=rng)
    for law in ("reference", "uniform"):
        ms, (prob, w) = timed(lambda: eng.exact_ext(q, e, law))
        print("%-34s %-9s %9.3f ms  equity %.6f  weights %s" % (name, law, ms, prob[0]["win"] + prob[0]["tie"],
                                                                 "yes" if w[0]["runs"] else "none"), flush=True)
for name, hero, board, n in [("plain heads-up preflop", ["AH", "KH"], [], 2), ("plain 3-way flop", ["9C", "8C"], ["7C", "6D", "2S"], 3)]:
    q = _lib.pack_query_one(ids(hero), ids(board), n, 1)
    ms, _ = timed(lambda: eng.exact(q, "reference"))
    print("%-34s %-9s %9.3f ms" % (name, "reference", ms), flush=True)
