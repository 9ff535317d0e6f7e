#!/usr/bin/env python3
"""The split-pot form of the extended kernels (mcq_eval_batch_ext_ways) timed beside the credited form, on the workloads
of tools/ext_probe.py: 2048 x 6-max x 20 000 runs with every class, top 50 % and top 25 %, and the one-launch call of
one ranged 1000-run query.  Kernel times are medians of the launches' own timestamps."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neuron_poker_amd as npa  # noqa: E402
from neuron_poker_amd import _lib  # noqa: E402
from tools.ext_probe import top  # noqa: E402


def main():
    eng = npa.Engine(0, kernel_times=True)
    g = np.random.default_rng(7)
    B, N, runs = 2048, 6, 20000
    cards = np.array([g.permutation(52)[:8] for _ in range(B)], np.uint8)
    q = npa.pack_queries(cards[:, :2], np.full((B, 5), 255, np.uint8), N, runs)

    def kernel_ms(f, reps=5):
        f()
        ms = []
        for _ in range(reps):
            f()
            ms.append(eng.last_kernel_ms)
        return float(np.median(ms))

    for name, ext in [("every class", _lib.pack_query_ext(B)), ("opponents top 50 %", _lib.pack_query_ext(B, opp_range=top(0.5))),
                      ("opponents top 25 %", _lib.pack_query_ext(B, opp_range=top(0.25)))]:
        a = kernel_ms(lambda: eng.eval_batch_ext(q, ext, 1))
        b = kernel_ms(lambda: eng.eval_batch_ext_ways(q, ext, 1))
        print("%-22s credited %8.3f ms   ways %8.3f ms   ratio %.3f" % (name, a, b, b / a))
    q1 = npa.pack_queries(cards[:1, :2], np.full((1, 5), 255, np.uint8), N, 1000)
    e1 = _lib.pack_query_ext(1, opp_range=top(0.25))
    eng.set_kernel_timing(False)
    for name, f in [("credited", lambda: eng.eval_batch_ext(q1, e1, 1)), ("ways", lambda: eng.eval_batch_ext_ways(q1, e1, 1))]:
        for _ in range(200):
            f()
        t0 = time.perf_counter()
        for _ in range(2000):
            f()
        print("one ranged 1000-run query, one launch, %-8s %.1f us per call" % (name, (time.perf_counter() - t0) / 2000 * 1e6))


if __name__ == "__main__":
    main()
