#!/usr/bin/env python3
"""Rank-sum hash of the plain path (csrc/mcq_device.hpp, "rank-sum hash"): feasibility and fixture.

    python tools/sum_hash.py            check the committed weights and split, print sizes and load factor
    python tools/sum_hash.py --search   greedy search for rank weights (smallest next weight that keeps the sums of all
                                        multisets of up to seven cards with equal card counts distinct)
    python tools/sum_hash.py --fixture  write tests/golden/sum_hash.json (id and type counts, sizes)

The tables themselves are built by mcq_fill_tables (deterministic C++: first-fit-decreasing over the rows); this tool
reads them through the test-only host build tests/hostsim_sum, so what it reports is what a context creates.
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LDS_BUDGET = 144 * 1024   # 160 KB per CU minus the base decks (16 KB), sel8 (1 KB) and the small words


def count_vectors():
    """all (c_0..c_12), 0 <= c_r <= 4, sum 7"""
    out = []

    def rec(r, left, cur):
        if r == 13:
            if left == 0:
                out.append(tuple(cur))
            return
        for c in range(min(4, left) + 1):
            rec(r + 1, left - c, cur + [c])
    rec(0, 7, [])
    return np.array(out, np.int64)


def sums_distinct(w):
    s = count_vectors() @ np.asarray(w, np.int64)
    return len(s), len(np.unique(s)), int(s.max())


def search():
    """greedy: ranks one by one; partial multisets (<= 7 cards of the ranks so far) with EQUAL card counts must have
    distinct sums, so that any common completion keeps them apart"""
    w = [0]
    sets = {0: {0}}   # card count -> sums
    for c in range(1, 5):
        sets[c] = {0}
    for r in range(1, 13):
        cand = w[-1] + 1
        while True:
            new, ok = {}, True
            for c in range(8):
                acc = set()
                n = 0
                for j in range(min(4, c) + 1):
                    base = sets.get(c - j)
                    if base is None:
                        continue
                    acc.update(s + j * cand for s in base)
                    n += len(base)
                if len(acc) != n:
                    ok = False
                    break
                new[c] = acc
            if ok:
                break
            cand += 1
        w.append(cand)
        sets = new
        print("rank %2d weight %d" % (r, cand), flush=True)
    return w


def report():
    from tests import hostsim_sum as H
    i = H.info()
    hoff, hrank, tfid, tf = H.tables()
    w = H.weights()
    n, distinct, top = sums_distinct(w)
    used = int(np.count_nonzero(hrank))
    last = int(np.flatnonzero(hrank)[-1])
    ids = np.unique(np.concatenate([hrank[hrank != 0].astype(np.uint32), tfid[tfid != 0]]))
    return {"weights": [int(v) for v in w], "multisets": n, "distinct_sums": distinct, "largest_sum": top,
            "shift": i["shift"], "rows": i["rows"], "slots": i["slots"], "slots_used": used, "last_slot": last,
            "load_factor": round(used / (last + 1), 4), "hash_bytes": 2 * (i["rows"] + i["slots"]),
            "image_bytes": i["image_bytes"], "fits": i["fits"] and 2 * (i["rows"] + i["slots"]) <= LDS_BUDGET,
            "ids_by_code": i["ids_by_code"], "ids": int(len(ids))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--fixture", action="store_true")
    a = ap.parse_args()
    if a.search:
        w = search()
        print("weights", w, "-> multisets, distinct sums, largest sum:", sums_distinct(w))
        return
    r = report()
    print(json.dumps(r, indent=1))
    if a.fixture:
        with open(os.path.join(ROOT, "tests", "golden", "sum_hash.json"), "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
