#!/usr/bin/env python3
"""Timing of mcq_exact_matrix / mcq_exact_matrix_device beside the two ways to the same numbers that the library had before:

  (i)  one mcq_exact_batch_seats record per unordered pair of hands of the flop (635 628 records, in calls of 65 535);
  (ii) one mcq_exact_batch_hero_range_weighted record per opponent hand with a one-hot weight table (1176 records, in calls
       of 1024, the hero's table holding the hands that can meet it): its win and tie columns are a column of the matrices.

    python tools/matrix_probe.py [--rounds N] [--baseline-rounds N]

Every way is checked against the matrices before anything is timed.  Call times: host clock around calls that end in a
synchronise, medians of alternating rounds after a warm-up of every shape, min and max stated.  Kernel times:
mcq_set_kernel_timing's timestamp events of the three kernels of a call (ranking, counting, finish), on an engine of their
own -- the timestamped launches cost a call a few microseconds each.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP, TURN, RIVER = ["AH", "KD", "7C"], ["AS", "9D", "9H", "QC"], ["9C", "9D", "KH", "KS", "AC"]


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return "median %9.3f ms  (min %9.3f, max %9.3f, n %d)" % (np.median(ts), ts.min(), ts.max(), len(ts))


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--baseline-rounds", type=int, default=2)
    a = ap.parse_args()
    import torch
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    eng, eng_t = npa.Engine(0), npa.Engine(0, kernel_times=True)
    rec = {name: _lib.pack_matrix_query([npa.card_id(c) for c in cards]) for name, cards in
           (("flop_full", FLOP), ("turn", TURN), ("river", RIVER))}
    rows = _lib.HAND_ROWS
    dev = torch.device("cuda", 0)
    d_win = torch.empty((64, rows, rows), dtype=torch.int16, device=dev)
    d_tie = torch.empty_like(d_win)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def device_call(e, q):
        e.exact_matrix_device(q, d_win.data_ptr(), d_tie.data_ptr(), stream=stream)
        torch.cuda.synchronize(dev)

    # ---- the matrices, and the device entry's bytes against the host entry's
    win, tie, total = eng.exact_matrix(rec["flop_full"])
    win, tie, total = win[0], tie[0], int(total[0])
    device_call(eng, rec["flop_full"])
    assert np.array_equal(d_win[0].cpu().numpy().view(np.uint16), win) and np.array_equal(d_tie[0].cpu().numpy().view(np.uint16), tie)
    board = [npa.card_id(c) for c in FLOP]
    deck = [c for c in range(52) if c not in board]
    hands = sorted(((x, y) for i, x in enumerate(deck) for y in deck[i + 1:]), key=lambda h: _lib.hand_index(*h))
    idx = np.array([_lib.hand_index(*h) for h in hands])
    print("flop %s: %d hands, total %d, pairs with a tie %d, win == total %d" %
          (" ".join(FLOP), len(hands), total, int((tie > 0).sum()) // 2, int((win == total).sum())), flush=True)

    # ---- (ii) one-hot opponent tables through the weighted hero-range entry
    q1 = _lib.pack_query_one([0, 0], board, 2, 1)
    x1 = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES)
    h = np.array(hands, np.uint8)
    apart = ((h[:, None, 0] != h[None, :, 0]) & (h[:, None, 0] != h[None, :, 1]) &
             (h[:, None, 1] != h[None, :, 0]) & (h[:, None, 1] != h[None, :, 1]))
    onehot = np.zeros((len(hands), rows), np.uint16)
    onehot[np.arange(len(hands)), idx] = 1
    hero_w = np.zeros((len(hands), rows), np.uint16)       # the hero hands that can meet that opponent hand: the entry refuses a
    hero_w[:, idx] = apart                                 # hero hand against which the opponent's range cannot be dealt

    def way_weighted(check=False):
        for lo in range(0, len(hands), 1024):
            n = min(1024, len(hands) - lo)
            r, _ = eng.exact_hero_range_weighted(np.repeat(q1, n), np.repeat(x1, n), onehot[lo:lo + n], hero_w[lo:lo + n])
            if check:
                assert np.array_equal(r["win"], win[:, idx[lo:lo + n]].T) and np.array_equal(r["tie"], tie[:, idx[lo:lo + n]].T)

    # ---- (i) one all-in record per unordered pair of hands
    pi, pj = np.nonzero(np.triu(apart, 1))
    assert len(pi) == 635628
    b5 = np.full((len(pi), 5), 255, np.uint8)
    b5[:, :3] = board
    q_all = _lib.pack_queries(h[pi], b5, 2, 1)
    x_all = _lib.pack_query_ext(len(pi))
    x_all["n_known"] = 1
    x_all["known"]["cards"][:, 0] = h[pj]

    def way_seats(check=False):
        for lo in range(0, len(pi), 65535):
            hi = min(lo + 65535, len(pi))
            r = eng.exact_seats(q_all[lo:hi], x_all[lo:hi], law="uniform")
            if check:
                a, b = idx[pi[lo:hi]], idx[pj[lo:hi]]
                assert np.array_equal(r["seat"]["win"][:, 0], win[a, b]) and np.array_equal(r["seat"]["win"][:, 1], win[b, a])
                assert np.array_equal(r["seat"]["tie"][:, 0], tie[a, b]) and (r["runs"] == total).all()

    way_weighted(check=True)
    way_seats(check=True)
    print("both older ways give the matrices' entries: checked on all 1176 columns and all 635 628 pairs", flush=True)

    # ---- call times, alternating rounds
    batch64 = np.repeat(rec["flop_full"], 64)
    ways = [("host entry", lambda q: eng.exact_matrix(q)), ("device entry", lambda q: device_call(eng, q))]
    for name in rec:                                   # warm-up of every shape, both entries, both engines
        for _, f in ways:
            f(rec[name])
        device_call(eng_t, rec[name])
    device_call(eng, batch64)
    device_call(eng_t, batch64)
    t = {(name, w): [] for name in rec for w, _ in ways}
    t64, kern, kern64 = [], {name: [] for name in rec}, []
    for _ in range(a.rounds):
        for name in rec:
            for w, f in ways:
                t[(name, w)].append(timed(lambda: f(rec[name])))
            device_call(eng_t, rec[name])
            kern[name].append(eng_t.kernel_times(3).copy())
        t64.append(timed(lambda: device_call(eng, batch64)))
        device_call(eng_t, batch64)
        kern64.append(eng_t.kernel_times(12).reshape(4, 3).sum(0))
    for name in rec:
        for w, _ in ways:
            print("%-10s %-13s call   %s" % (name, w, stats(t[(name, w)])))
        k = np.array(kern[name])
        print("%-10s %-13s kernel ranking %.3f ms, counting %.3f ms, finish %.3f ms, sum %.3f ms (medians of %d; sum min %.3f, max %.3f)" %
              (name, "device entry", *np.median(k, 0), np.median(k.sum(1)), len(k), k.sum(1).min(), k.sum(1).max()))
    k = np.array(kern64)
    print("64 flops   device entry  call   %s  = %.3f ms per flop" % (stats(t64), np.median(t64) * 1e3 / 64))
    print("64 flops   device entry  kernel ranking %.3f ms, counting %.3f ms, finish %.3f ms, sum %.3f ms (four launch groups of 16)" %
          (*np.median(k, 0), np.median(k.sum(1))))

    # ---- the baselines, alternating with the new call
    tw, ts_, tn = [], [], []
    for _ in range(a.baseline_rounds):
        tw.append(timed(way_weighted))
        tn.append(timed(lambda: eng.exact_matrix(rec["flop_full"])))
        ts_.append(timed(way_seats))
        tn.append(timed(lambda: eng.exact_matrix(rec["flop_full"])))
    print("baseline (ii) weighted one-hot, 1176 records: %s" % stats(tw))
    print("baseline (i)  all-in pairs, 635628 records:   %s" % stats(ts_))
    print("new host entry between them:                  %s" % stats(tn))
    base, new_host, new_dev = min(np.median(tw), np.median(ts_)), np.median(t[("flop_full", "host entry")]), \
        np.median(t[("flop_full", "device entry")])
    kf = np.median(np.array(kern["flop_full"]), 0)
    print("flop_full: baseline %.1f ms (the faster: %s) / host entry %.3f ms = %.0fx; / device entry %.3f ms = %.0fx" %
          (base * 1e3, "(ii)" if np.median(tw) <= np.median(ts_) else "(i)", new_host * 1e3, base / new_host, new_dev * 1e3,
           base / new_dev))
    print("flop_full: the count kernel is %.0f %% of the device entry's call and %.0f %% of its kernel time" %
          (100 * kf[1] / (new_dev * 1e3), 100 * kf[1] / kf.sum()))
    pair_completions = 1176.0 * 1176.0 * 1176.0
    print("flop_full: %.3g compare-adds in %.3f ms of counting = %.3g per second" % (pair_completions, kf[1], pair_completions / (kf[1] * 1e-3)))
    eng.close()
    eng_t.close()


if __name__ == "__main__":
    main()
