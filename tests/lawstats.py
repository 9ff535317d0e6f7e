"""Statistics shared by the dealing-law tests (tests/test_dealing_law_*.py): is a tally row -- or the sum of many -- drawn
from a given law?

A tally row is the 13 integers of mcq_result / the oracle's out[13]: runs, passes, win, tie, by_type[9].  Every check
covers eleven statistics: the strict-win share, the tie share and the nine shares of hero's winning hand types.

* one_sample(rows, prob): the rows against exact probabilities (Engine.exact_ext, mcq_exact_batch weights);
  sigma = sqrt(p (1 - p) / n), floored at 1 / n so that a share near 0 or 1 still has a scale.
* two_sample(rows1, rows2): two Monte-Carlo runs of what should be the same law;
  sigma = sqrt(p1 (1 - p1) / n1 + p2 (1 - p2) / n2), floored at 1 / min(n1, n2).

One bound for every test, BOUND = 5.5 sigma: each test makes tens to hundreds of comparisons, and at 5.5 sigma a
correct law fails one of a thousand of them with probability below 4e-5.  The seeds are fixed, so a run is
deterministic; a failure is a finding about the law, never a reason to widen the bound.

`passes` is NOT compared: the production streams (MCQ-CTR) spend one word per opponent dealt by index and one per trial
on a candidate list, while the reference re-draws index pairs (r1, r2) until r1 != r2 and the range allows the pair, so
the two count different things under the same law.
"""
import numpy as np

BOUND = 5.5
TYPES = ["HighCard", "Pair", "TwoPair", "ThreeOfAKind", "Straight", "Flush", "FullHouse", "FourOfAKind", "StraightFlush"]
NAMES = ["win", "tie"] + TYPES


def counts(rows):
    """rows: RESULT_DTYPE records, uint64 [.., 13] rows or one run_ex dict -> (n, the eleven counts as int)."""
    if isinstance(rows, dict):
        rows = rows["tallies"]
    a = np.ascontiguousarray(rows)
    if a.dtype.names:
        a = a.view(np.uint64)
    t = a.reshape(-1, 13).astype(np.uint64).sum(0, dtype=np.uint64)
    return int(t[0]), [int(t[2]), int(t[3])] + [int(x) for x in t[4:13]]


def exact_vector(prob):
    """EXACT_PROB_DTYPE record (win, tie, by_type[9]) or any sequence of eleven numbers -> eleven floats."""
    if getattr(prob, "dtype", None) is not None and prob.dtype.names:
        return [float(prob["win"]), float(prob["tie"])] + [float(x) for x in prob["by_type"]]
    v = [float(x) for x in prob]
    assert len(v) == 11, len(v)
    return v


def one_sample(rows, prob):
    """-> [(statistic, observed, exact, z)] of the rows against exact probabilities."""
    n, c = counts(rows)
    assert n > 0
    out = []
    for name, k, p in zip(NAMES, c, exact_vector(prob)):
        sigma = max((p * (1.0 - p) / n) ** 0.5, 1.0 / n)
        out.append((name, k / n, p, (k / n - p) / sigma))
    return out


def two_sample(rows1, rows2):
    """-> [(statistic, share 1, share 2, z)] of two tally sets."""
    n1, c1 = counts(rows1)
    n2, c2 = counts(rows2)
    assert n1 > 0 and n2 > 0
    out = []
    for name, k1, k2 in zip(NAMES, c1, c2):
        p1, p2 = k1 / n1, k2 / n2
        sigma = max((p1 * (1.0 - p1) / n1 + p2 * (1.0 - p2) / n2) ** 0.5, 1.0 / min(n1, n2))
        out.append((name, p1, p2, (p1 - p2) / sigma))
    return out


def max_z(result):
    return max(abs(r[3]) for r in result)


def report(label, result):
    """One line per check: the largest |z| and the statistic it belongs to."""
    worst = max(result, key=lambda r: abs(r[3]))
    return "%s: max |z| %.2f (%s: %.7f vs %.7f)" % (label, abs(worst[3]), worst[0], worst[1], worst[2])


def check(label, result, bound=BOUND):
    """Print the report line and assert every |z| <= bound; the message lists each statistic beyond it."""
    print(report(label, result))
    bad = ["%s: %.7f vs %.7f, z = %+.2f" % r for r in result if not abs(r[3]) <= bound]
    assert not bad, "%s: beyond %.1f sigma: %s" % (label, bound, "; ".join(bad))
