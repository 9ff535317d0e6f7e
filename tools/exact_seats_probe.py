#!/usr/bin/env python3
"""Kernel time of the exact per-seat enumeration with one random opponent (mcq_exact_batch_ext_seats:
mcq_exact_ext_kernel<1, MCQ_ROW_SEATS>) beside the hero-only split-pot enumeration of the same records
(mcq_exact_batch_ext_ways: mcq_exact_ext_kernel<1, MCQ_ROW_WAYS>), in one process and one session.

    python3 tools/exact_seats_probe.py [out_dir]

starts itself once more under `rocprofv3 --kernel-trace` (a fresh process: this one never opens the GPU), reads the
kernel trace and prints, per record and law, the median of the kernels' own timestamps after the warm-up launches, and
the ratio of the two medians.  Records: AhKh + known QsQc against one top-25 % opponent, preflop and on a flop."""
import csv
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 3, 15
RECORDS = [("preflop", []), ("flop 2c7d9h", ["2C", "7D", "9H"])]
LAWS = ["reference", "uniform"]
ENTRIES = ["ext_ways", "ext_seats"]


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    eng = npa.Engine(0)
    ids = lambda cs: [npa.card_id(c) for c in cs]  # noqa: E731
    for _, board in RECORDS:
        q = _lib.pack_query_one(ids(["AH", "KH"]), ids(board), 3, 1)
        e = _lib.pack_query_ext(1, known=[ids(["QS", "QC"])], opp_range=_opponent_range_bits(0.25))
        for law in LAWS:
            for _ in range(WARM + REPS):
                _, ways = eng.exact_ext_ways(q, e, law)
            for _ in range(WARM + REPS):
                seats = eng.exact_ext_seats(q, e, law)
            w, s = ways.view(np.uint64).reshape(22), seats.view(np.uint64).reshape(32)
            assert [int(x) for x in s[:4]] == [int(x) for x in w[:4]], "seat 0 is the hero-only row"
    eng.close()


def main():
    out = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else "exact_seats_probe_out")
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable,
           os.path.abspath(__file__), "--child"]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if len(traces) != 1:
        raise SystemExit("expected one kernel trace under %s, found %d" % (out, len(traces)))
    with open(traces[0], newline="") as f:
        rows = [r for r in csv.DictReader(f) if "mcq_exact_ext_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    if len(rows) != per * len(RECORDS) * len(LAWS) * len(ENTRIES):
        raise SystemExit("%d launches of mcq_exact_ext_kernel in the trace, expected %d" % (len(rows), per * 8))
    print("median kernel time over %d launches after %d warm-up launches (rocprofv3 --kernel-trace timestamps)" % (REPS, WARM))
    at = 0
    for name, _ in RECORDS:
        for law in LAWS:
            med = []
            for entry in ENTRIES:
                part = rows[at:at + per]
                at += per
                names = {r["Kernel_Name"] for r in part}
                if len(names) != 1:
                    raise SystemExit("mixed kernels in one slice: %s" % names)
                us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part[WARM:]]
                med.append(statistics.median(us))
                print("%-12s %-9s %-9s median %10.1f us  min %10.1f  max %10.1f   %s" % (
                    name, law, entry, med[-1], min(us), max(us), names.pop()), flush=True)
            print("%-12s %-9s ext_seats / ext_ways = %.3f" % (name, law, med[1] / med[0]), flush=True)


if __name__ == "__main__":
    child() if "--child" in sys.argv[1:] else main()
