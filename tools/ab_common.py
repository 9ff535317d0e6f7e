"""The A/B loop of the refactor probes (tools/hero_preflop_weighted_probe.py --ab, tools/exact_ext_ab_probe.py): this
build of the library beside the parent commit's build and beside a second copy of the parent's build (the same file under
a second name, so that it loads separately) -- what a refactor of an entry must leave alone."""
import time

import numpy as np


def ab(make, paths, cases, passes, faster_fails):
    """make(path) opens one build of the library with a context of its own (and has .close()); paths = this build's, the
    parent's, the copy's.  cases: (key, rounds, call) with call(lib, slot) making the entry's call on `lib` into the
    output buffers `slot` (0, 1, 2) and returning them as a tuple of arrays; key is a tuple of strings (entry, shape).

    Per case the three libraries are called in turn, in one order and then in the reverse one, after a warm-up call whose
    outputs are checked to be equal byte for byte.  Per order: this / parent and copy / parent, the ratios of the median
    call times over `rounds` calls.  The same code differs by up to a percent and more between two CONTEXTS, steadily for as
    long as they live (the copy against the parent shows it), so the whole is done `passes` times, each with fresh contexts
    of all three libraries.  The copy / parent ratios of all passes and orders span the interval that the same code gives
    against itself; a case passes when every this / parent ratio lies in that interval widened on each side by its own
    width.  "faster" (the ratios outside lie below the interval) is printed, and fails like "OUTSIDE" where faster_fails.
    -> whether every case passed."""
    ratios = {key: [] for key, _, _ in cases}                           # (this / parent, copy / parent, parent ms) per pass and order
    for _p in range(passes):
        libs = list(zip(("this", "parent", "copy"), (make(p) for p in paths)))
        for key, rounds, call in cases:
            first = [call(b, slot) for slot, (_, b) in enumerate(libs)]  # warm-up, and the check
            assert all(len(o) == len(first[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(o, first[0])) for o in first), key
            for order in (libs, libs[::-1]):
                t = {k: [] for k, _ in libs}
                for _ in range(rounds):
                    for k, b in order:
                        t0 = time.perf_counter()
                        call(b, 0)
                        t[k].append((time.perf_counter() - t0) * 1e3)
                med = {k: float(np.median(v)) for k, v in t.items()}
                ratios[key].append((med["this"] / med["parent"], med["copy"] / med["parent"], med["parent"]))
        for _, b in libs:
            b.close()
        print("pass done", flush=True)
    ok = True
    for key, r in ratios.items():
        lo, hi = min(v[1] for v in r), max(v[1] for v in r)
        lo, hi = lo - (hi - lo), hi + (hi - lo)
        verdict = "inside" if all(lo <= v[0] <= hi for v in r) else "faster" if all(v[0] <= hi for v in r) else "OUTSIDE"
        ok = ok and (verdict == "inside" or (verdict == "faster" and not faster_fails))
        print("%-28s %-46s parent %9.3f ms  widened [%.4f, %.4f]  %s\n    this/parent %s\n    copy/parent %s" %
              (key[0], key[1], float(np.median([v[2] for v in r])), lo, hi, verdict, " ".join("%.4f" % v[0] for v in r),
               " ".join("%.4f" % v[1] for v in r)), flush=True)
    return ok
