#!/usr/bin/env python3
"""Timing of mcq_exact_batch_ext_runouts (the row of every table completion from one enumeration) beside the only other way
to the same rows, which exists under the uniform law only: per flop, ONE mcq_exact_batch_ext_ways call over the 1081 river
records that have both cards appended to the table.

    python tools/runout_probe.py          call times: a host clock around calls that end in a synchronise, the two ways
                                          alternating, after a warm-up of every shape

Shapes: one flop record against any hand (47 cards left, 1081 completions), and a batch of 169 such flops (one hero hand
per preflop class) -- the other way is then 169 calls.  Both ways are checked to give the same rows before anything is
timed."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP = ["QS", "7D", "2H"]
ROUNDS_ONE, ROUNDS_BATCH = 1000, 20


def class_hands(table):
    """One hero hand per preflop class (169), none of its cards on the table."""
    seen, hands = set(), []
    for b in range(52):
        for a in range(b):
            ra, rb = a >> 2, b >> 2
            cls = (ra, rb, ra != rb and (a & 3) == (b & 3))
            if cls not in seen and a not in table and b not in table:
                seen.add(cls)
                hands.append([a, b])
    assert len(hands) == 169
    return hands


def river_records(hero, table):
    from neuron_poker_amd import _lib
    deck = [c for c in range(52) if c not in table and c not in hero]
    hands = [(a, b) for b in deck for a in deck if a < b]
    q = np.concatenate([_lib.pack_query_one(hero, table + [a, b], 2, 1) for a, b in hands])
    return q, _lib.pack_query_ext(len(hands)), [_lib.hand_index(a, b) for a, b in hands]


def main():
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    eng = npa.Engine(0)
    table = [npa.card_id(c) for c in FLOP]
    heroes = class_hands(table)
    flops = np.concatenate([_lib.pack_query_one(h, table, 2, 1) for h in heroes])
    ext = _lib.pack_query_ext(len(heroes))
    rivers = [river_records(h, table) for h in heroes]
    for name, n, rounds in (("one flop record", 1, ROUNDS_ONE), ("169 flop records", 169, ROUNDS_BATCH)):
        def new():
            return eng.exact_ext_runouts(flops[:n], ext[:n], "uniform")

        def old():
            return [eng.exact_ext_ways(q, x, "uniform")[1] for q, x, _ in rivers[:n]]
        _, pairs = new()                                        # warm-up of this shape, and the check
        for i, (w, (_, _, idx)) in enumerate(zip(old(), rivers[:n])):
            assert len(idx) == 1081
            assert np.array_equal(pairs[i][idx].view(np.uint64), w.view(np.uint64)), (name, i)
        t_new, t_old = [], []
        for _ in range(rounds):                                 # alternating: what else runs on the host hits both alike
            t0 = time.perf_counter()
            new()
            t1 = time.perf_counter()
            old()
            t2 = time.perf_counter()
            t_new.append(t1 - t0)
            t_old.append(t2 - t1)
        mn, mo = np.median(t_new) * 1e3, np.median(t_old) * 1e3
        print("%-17s call: river records, %3d call(s) of 1081 %9.3f ms (min %9.3f)  runouts, one call %9.3f ms (min %9.3f)  ratio %5.1fx"
              % (name, n, mo, min(t_old) * 1e3, mn, min(t_new) * 1e3, mo / mn), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
