#!/usr/bin/env python3
"""What the split-pot rows cost: mcq_eval_batch_device_ways against mcq_eval_batch_device on the
headline workload of bench.py (6-max before the flop, 4096 x 100 000, HBM-resident), and one 1000-run query through
mcq_eval_batch_ways against mcq_eval_batch -- both pairs in one process, calls interleaved.

    python tools/ways_probe.py [--reps 30] [--small-reps 2000]

Bulk: the evaluation kernel's own begin/end timestamps (mcq_set_kernel_timing); after 5 warm-up pairs the MEDIAN and the
minimum over --reps interleaved pairs.  Small query: wall time per call, median of --small-reps after 200 warm-up calls."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neuron_poker_amd as npa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small-reps", type=int, default=2000)
    ap.add_argument("--states", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100000)
    a = ap.parse_args()
    import torch
    eng = npa.Engine(0, kernel_times=True)
    g = np.random.default_rng(4096)
    hole = np.array([g.choice(52, 2, replace=False) for _ in range(a.states)], np.uint8)
    q = npa.pack_queries(hole, np.full((a.states, 5), 255, np.uint8), 6, a.iters)
    dq = torch.from_numpy(q.view(np.uint8).reshape(-1, 16).copy()).cuda()
    plain = torch.empty((a.states, 13), dtype=torch.int64, device="cuda")
    ways = torch.empty((a.states, 22), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    t = {"plain": [], "ways": []}
    for i in range(5 + a.reps):
        for name, fn, out in (("plain", eng.eval_batch_device, plain), ("ways", eng.eval_batch_device_ways, ways)):
            fn(dq.data_ptr(), a.states, 1, out.data_ptr(), first_query_id=0, stream=s)
            torch.cuda.synchronize()
            if i >= 5:
                t[name].append(eng.last_kernel_ms)
    assert torch.equal(plain, ways[:, :13]) and torch.equal(ways[:, 13:].sum(1), ways[:, 3])
    mp, mw = np.median(t["plain"]), np.median(t["ways"])
    print("bulk %d x %d, 6-max preflop, kernel ms: plain median %.4f min %.4f | ways median %.4f min %.4f | ratio of medians "
          "%.4f, of minima %.4f (%d interleaved pairs)" % (a.states, a.iters, mp, min(t["plain"]), mw, min(t["ways"]), mw / mp,
                                                          min(t["ways"]) / min(t["plain"]), a.reps))
    eng.close()
    eng = npa.Engine(0)   # (no kernel timing: a timestamped launch costs a small query microseconds)
    q1 = npa.pack_queries([[50, 46]], [[255] * 5], 6, 1000)
    w = {"plain": [], "ways": []}
    for i in range(200 + a.small_reps):
        for name, fn in (("plain", eng.eval_batch), ("ways", eng.eval_batch_ways)):
            t0 = time.perf_counter()
            fn(q1, 1, first_query_id=i)
            dt = time.perf_counter() - t0
            if i >= 200:
                w[name].append(dt * 1e6)
    print("one 1000-run 6-max query, host entry, us per call: plain median %.2f min %.2f | ways median %.2f min %.2f | "
          "difference of medians %.2f us (%d interleaved pairs)" % (np.median(w["plain"]), min(w["plain"]), np.median(w["ways"]),
                                                                   min(w["ways"]), np.median(w["ways"]) - np.median(w["plain"]),
                                                                   a.small_reps))
    eng.close()


if __name__ == "__main__":
    main()
