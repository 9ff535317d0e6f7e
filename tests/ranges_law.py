"""The law of the weighted-range-per-seat Monte-Carlo entry (mcq_ranges.hpp, "MCQ-RG v1") as exact numbers, from code
that shares nothing with the lane code: pure Python integers and fractions over small supports.

    P(h_0, .., h_{p-1})  ~  prod_s eff_s(h_s) * [pairwise disjoint],   then the missing table cards uniformly,

eff_s = the seat's weights restricted to the hands clear of the table.  A case is a table of 0/3/4/5 cards and, per seat,
a small support {hand: weight}; cards are '2C' .. 'AS', ids 4 * rank + suit.

    tuples(supports, board)            every disjoint tuple with its integer weight, and the acceptance probability a
    expect_from_all_in(tuples, rows)   per seat P(win), P(tie), E[share / UNIT] from the ALL-IN row of every tuple
    sequential_law(supports, board)    the tuples under the wrong law that is cheapest to fall into
    z_rows(row, expect, a, n)          a Monte-Carlo row against the expectation, for tests/lawstats.check
    conditions(...)                    what a case must satisfy to test anything, asserted

The all-in rows are 32-word per-seat rows (runs, passes, then win, tie, share of seat 0..9): Engine.exact_seats writes
them on the GPU, all_in_rows() below builds them on the CPU with the oracle's scorer (river, turn and flop tables).
"""
import itertools
from fractions import Fraction

import numpy as np

from oracle import oracle as O

UNIT = 2520
RANKS, SUITS = "23456789TJQKA", "CDHS"
COUNT_MIN = 100   # a compared probability is exactly 0 or expects at least this many events
SEQ_GAP = 10.0    # the sequential law must lie at least this many sigma from the joint law in one statistic
ACCEPT_MIN = Fraction(1, 4)


def cid(s):
    return 4 * RANKS.index(s[0]) + SUITS.index(s[1])


def cname(c):
    return RANKS[c >> 2] + SUITS[c & 3]


def hand(s):
    """'AsKh' style is not used here: 'ASKH' -> (a, b), a < b."""
    a, b = cid(s[:2]), cid(s[2:])
    return (min(a, b), max(a, b))


def hidx(h):
    return h[1] * (h[1] - 1) // 2 + h[0]


def table(support):
    """{hand string: weight} -> uint16 [1326]"""
    t = np.zeros(1326, np.uint16)
    for s, w in support.items():
        t[hidx(hand(s))] = w
    return t


def wide(weight):
    """Every one of the 1326 hands at one weight."""
    return {cname(a) + cname(b): weight for b in range(52) for a in range(b)}


def joint_law(supports, board):
    """The specification, literally: {(h_0, .., h_{p-1}): probability} over the deals of positive weight."""
    B = {cid(c) for c in board}
    eff = [[(hand(s), w) for s, w in sup.items() if w and not (set(hand(s)) & B)] for sup in supports]
    law = {}
    for combo in itertools.product(*eff):
        cards = [c for h, _ in combo for c in h]
        if len(set(cards)) == len(cards):
            law[tuple(h for h, _ in combo)] = float(np.prod([w for _, w in combo]))
    z = sum(law.values())
    return {k: v / z for k, v in law.items()}


def literal_rows(supports, board, exact=False):
    """Per seat (P(win), P(tie), E[share / UNIT], Var[share / UNIT] per iteration) from the literal enumeration of the joint
    law and of every completion of the table, scored with the oracle's scorer.  exact=True: the same four as Fractions,
    from the integer weights of the deals (every deal has the same number of completions)."""
    p = len(supports)
    B = [cid(c) for c in board]
    if exact:
        eff = [{hand(s): int(w) for s, w in sup.items() if w} for sup in supports]
        law = {k: int(np.prod([eff[s][h] for s, h in enumerate(k)], dtype=object)) for k in joint_law(supports, board)}
    else:
        law = joint_law(supports, board)
    keys, seven, wts = list(law), [], []
    for k in keys:
        used = set(B) | {c for h in k for c in h}
        rest = [c for c in range(52) if c not in used]
        comps = list(itertools.combinations(rest, 5 - len(B)))
        for comp in comps:
            for h in k:
                seven.append(list(h) + B + list(comp))
            wts.append(law[k] if exact else law[k] / len(comps))
    sc = O.score_batch(np.array(seven, np.uint8), 4).reshape(-1, p)
    best = sc.max(1, keepdims=True)
    level = sc == best
    kk = level.sum(1, keepdims=True)
    if exact:
        tot = sum(wts)
        out = []
        for s in range(p):
            win = sum(w for w, l, k in zip(wts, level[:, s], kk[:, 0]) if l and k == 1)
            tie = sum(w for w, l, k in zip(wts, level[:, s], kk[:, 0]) if l and k > 1)
            m = sum(Fraction(w, int(k)) for w, l, k in zip(wts, level[:, s], kk[:, 0]) if l) / tot
            m2 = sum(Fraction(w, int(k) ** 2) for w, l, k in zip(wts, level[:, s], kk[:, 0]) if l) / tot
            out.append((Fraction(win, tot), Fraction(tie, tot), m, m2 - m * m))
        return out
    wts = np.array(wts)
    win = (level & (kk == 1)).astype(float)
    tie = (level & (kk > 1)).astype(float)
    share = level / kk
    out = []
    for s in range(p):
        m = float((wts * share[:, s]).sum())
        out.append((float((wts * win[:, s]).sum()), float((wts * tie[:, s]).sum()), m,
                    float((wts * share[:, s] ** 2).sum()) - m * m))
    return out


# ---------------------------------------------------------------------------------------------------- the law in integers
def _eff(supports, board):
    B = {cid(c) for c in board}
    eff = [[(hand(s), int(w)) for s, w in sup.items() if w and not (set(hand(s)) & B)] for sup in supports]
    assert all(eff), "a seat without a hand clear of the table"
    return eff


def tuples(supports, board):
    """-> ([(hands, weight)], a): every tuple of pairwise disjoint hands clear of the table, seat by seat in the order of
    the supports, with its integer weight prod_s w_s(h_s), and the exact probability that a whole trial is accepted,
    a = sum of the tuple weights / prod_s (sum of eff_s), as a Fraction."""
    eff = _eff(supports, board)
    out = []

    def walk(s, used, hs, wt):
        if s == len(eff):
            out.append((tuple(hs), wt))
            return
        for h, w in eff[s]:
            if not (used & ((1 << h[0]) | (1 << h[1]))):
                walk(s + 1, used | (1 << h[0]) | (1 << h[1]), hs + [h], wt * w)
    walk(0, 0, [], 1)
    assert out, "no disjoint tuple"
    den = 1
    for e in eff:
        den *= sum(w for _, w in e)
    return out, Fraction(sum(w for _, w in out), den)


def sequential_law(supports, board):
    """-> [(hands, probability)] over the same tuples in the same order, under the WRONG law: seat s draws from what the
    seats before it left (only the colliding seat draws again), so a tuple has probability
    prod_s w_s(h_s) / (weight of seat s's hands disjoint from h_0 .. h_{s-1}).  Feed it to expect_from_all_in in the
    place of tuples(): it exists only to show that a case can tell the two laws apart."""
    eff = _eff(supports, board)
    out = []

    def walk(s, used, hs, pr):
        if s == len(eff):
            out.append((tuple(hs), pr))
            return
        left = [(h, w) for h, w in eff[s] if not (used & ((1 << h[0]) | (1 << h[1])))]
        z = sum(w for _, w in left)
        for h, w in left:
            walk(s + 1, used | (1 << h[0]) | (1 << h[1]), hs + [h], pr * Fraction(w, z))
    walk(0, 0, [], Fraction(1))
    z = sum(pr for _, pr in out)   # (below 1 only where a seat is left without a hand: that mass never ends)
    return [(hs, pr / z) for hs, pr in out]


def words(row):
    return [int(x) for x in np.ascontiguousarray(row).view(np.uint64).reshape(32)]


def expect_from_all_in(tl, rows):
    """tl: [(hands, weight)] (integers or Fractions), rows: the all-in per-seat row of every tuple, in the same order
    -> [(P(win), P(tie), E[share / UNIT])] per seat, as Fractions."""
    assert len(tl) == len(rows) > 0
    rows = [words(r) for r in rows]
    runs = rows[0][0]
    assert runs > 0 and all(r[0] == runs for r in rows), "the tuples of one case have the same number of completions"
    p = len(tl[0][0])
    tot = sum(w for _, w in tl)
    out = []
    for s in range(p):
        win = sum(w * r[2 + 3 * s] for (_, w), r in zip(tl, rows))
        tie = sum(w * r[3 + 3 * s] for (_, w), r in zip(tl, rows))
        share = sum(w * r[4 + 3 * s] for (_, w), r in zip(tl, rows))
        out.append((Fraction(win) / (tot * runs), Fraction(tie) / (tot * runs), Fraction(share) / (tot * runs * UNIT)))
    assert sum(e[2] for e in out) == 1
    return out


def all_in_rows(tl, board):
    """(CPU) the 32-word all-in row of every tuple over every completion of the table, with the oracle's scorer."""
    B = [cid(c) for c in board]
    p = len(tl[0][0])
    out = np.zeros((len(tl), 32), np.uint64)
    for i, (hs, _) in enumerate(tl):
        used = set(B) | {c for h in hs for c in h}
        rest = [c for c in range(52) if c not in used]
        k = 5 - len(B)
        comps = np.array(list(itertools.combinations(rest, k)), np.uint8).reshape(-1, k) if k else np.zeros((1, 0), np.uint8)
        n = len(comps)
        seven = np.zeros((n, p, 7), np.uint8)
        for s, h in enumerate(hs):
            seven[:, s, 0], seven[:, s, 1] = h
        seven[:, :, 2:2 + len(B)] = B
        seven[:, :, 2 + len(B):] = comps[:, None, :]
        sc = O.score_batch(seven.reshape(-1, 7), 4).reshape(n, p)
        level = sc == sc.max(1, keepdims=True)
        kk = level.sum(1)
        out[i, 0] = n
        for s in range(p):
            out[i, 2 + 3 * s] = int((level[:, s] & (kk == 1)).sum())
            out[i, 3 + 3 * s] = int((level[:, s] & (kk > 1)).sum())
            out[i, 4 + 3 * s] = int((UNIT // kk[level[:, s]]).sum())
    return out


def _sigmas(e, n):
    """The three scales of one seat's (P(win), P(tie), E[share]) at n iterations.  Win and tie are binomial.  The share of
    an iteration is not Bernoulli and the all-in rows do not hold its second moment: a tied share is at most 1/2, so
    E[s^2] <= P(win) + (E[s] - P(win)) / 2, an upper bound of the variance -- conservative, it cannot raise a false alarm."""
    pw, pt, es = (float(x) for x in e)
    var = pw + (es - pw) / 2.0 - es * es
    return [max((q * (1.0 - q) / n) ** 0.5, 1.0 / n) for q in (pw, pt)] + [max((max(var, 0.0) / n) ** 0.5, 1.0 / n)]


def conditions(supports, board, tl, a, rows, n):
    """What a case must satisfy at n iterations, so that it cannot quietly stop testing anything -> the joint law's
    expectation [(P(win), P(tie), E[share])] per seat."""
    expect = expect_from_all_in(tl, rows)
    assert a >= ACCEPT_MIN, "acceptance %s: more than about four trials per iteration" % a
    for s, e in enumerate(expect):
        for name, q in (("win", e[0]), ("tie", e[1])):
            assert q == 0 or q * n >= COUNT_MIN, "seat %d %s: %.3g expected events at n = %d" % (s, name, float(q) * n, n)
    assert any(e[0] > 0 for e in expect) and any(e[1] > 0 for e in expect), "no strict win or no tie in the case"
    if sum(1 for e in _eff(supports, board) if len(e) > 1) >= 2:
        gap = sequential_gap(supports, board, expect, rows, n)
        assert gap >= SEQ_GAP, "the sequential law is only %.1f sigma away at n = %d" % (gap, n)
    return expect


def sequential_gap(supports, board, expect, rows, n):
    """The largest distance, in sigma of the joint law at n iterations, between the two laws' expectations."""
    wrong = expect_from_all_in(sequential_law(supports, board), rows)
    return max(abs(float(w[j]) - float(e[j])) / sg[j]
               for e, w in zip(expect, wrong) for sg in [_sigmas(e, n)] for j in range(3))


def z_rows(row, expect, a, n):
    """One Monte-Carlo row of n iterations against the expectation -> [(statistic, observed, exact, z)] for
    tests/lawstats.check: every seat's win, tie and share, and the whole trials per iteration, which are geometric:
    passes / n against 1 / a with sigma sqrt((1 - a) / a^2 / n).  When a == 1 no trial is ever abandoned: passes == runs."""
    r = words(row)
    assert r[0] == n
    out = []
    for s, e in enumerate(expect):
        sg = _sigmas(e, n)
        for j, name in enumerate(("win", "tie", "share")):
            got = r[2 + 3 * s + j] / (n * (UNIT if j == 2 else 1))
            if j < 2:
                assert e[j] == 0 or e[j] * n >= COUNT_MIN, (s, name)
                if e[j] == 0:
                    assert r[2 + 3 * s + j] == 0, "seat %d: a %s of probability zero was counted" % (s, name)
            out.append(("seat %d %s" % (s, name), got, float(e[j]), (got - float(e[j])) / sg[j]))
    if a == 1:
        assert r[1] == n, "no trial can be abandoned, yet passes = %d for %d runs" % (r[1], n)
    else:
        assert a >= ACCEPT_MIN
        af = float(a)
        out.append(("trials", r[1] / n, 1.0 / af, (r[1] / n - 1.0 / af) / ((1.0 - af) / (af * af) / n) ** 0.5))
    return out


# ------------------------------------------------------------------------------------------------------------- the cases
def case_tables(supports):
    """-> (uint16 [n_tables, 1326], the seats' table numbers): seats that hold the SAME dict name one table."""
    uniq, st = [], []
    for sup in supports:
        k = next((i for i, u in enumerate(uniq) if u is sup), None)
        if k is None:
            uniq.append(sup)
            k = len(uniq) - 1
        st.append(k)
    return np.stack([table(u) for u in uniq]), st


def _case(board, supports):
    return {"board": board.split(), "supports": supports}


_L2A = {"KHJD": 3, "8D6D": 1, "KS7H": 9, "JCTD": 7, "JHTH": 9}
# The smallest shapes at which the law can still go wrong.  Pairs, suited hands that make flushes on the table, hands that
# play the board and hands that two seats both hold; weights 1..9 unless the case is about the weight itself.  Every case
# satisfies conditions() at n = 2^20, L1, L2 and H6 at n = 200 000 as well (the host tests' n).
CASES = {
    # river, 3 seats, 8 hands each: the table holds a king-high straight that many hands only play
    "L1": _case("9S TH JH QH KD", [
        {"KSQC": 3, "8S2D": 1, "KH8C": 9, "JDTS": 7, "JSJC": 9, "AC8H": 1, "AD9D": 1, "ASQS": 2},
        {"9H2C": 3, "9C2H": 2, "QDTD": 6, "AH8D": 9, "KCTC": 7, "KS2S": 7, "9D9C": 5, "AH2D": 4},
        {"9C8H": 6, "QS9H": 9, "AH8D": 6, "KH9H": 3, "2H2D": 4, "QS2S": 3, "9C2H": 4, "ADJD": 7}]),
    # turn, 4 seats, 5 hands each; seats 0 and 2 name the SAME table
    "L2": _case("7C 8C 9D TC", [
        _L2A,
        {"JS6C": 8, "JCTD": 7, "9S6H": 3, "9C6S": 2, "KDTS": 6},
        _L2A,
        {"AS9H": 9, "ADAC": 7, "KC7D": 7, "AH8H": 5, "8S7S": 5}]),
    # flop, 6 seats, 3 hands each
    "L3": _case("5H 6H 7S", [
        {"KH9C": 3, "5D3D": 1, "KD4D": 9},
        {"AH9H": 5, "KC5C": 1, "7H3C": 7},
        {"AC3S": 5, "AS7C": 1, "KH5C": 6},
        {"AD6S": 9, "9S8D": 7, "8S4C": 7},
        {"KS5S": 5, "9D3H": 4, "6C4S": 6},
        {"8C6D": 9, "8H7D": 1, "KC6D": 3}]),
    # flop, 10 seats, 2 hands each
    "L4": _case("4D JS QC", [
        {"QSTC": 3, "5S2D": 1},
        {"AC9S": 6, "9D8H": 9},
        {"TD2C": 8, "9D8H": 7},
        {"8D2H": 3, "6S3C": 2},
        {"TS8C": 6, "AS7D": 9},
        {"KSJC": 7, "KC3S": 7},
        {"6C5H": 5, "AD3D": 4},
        {"6D5C": 6, "JH7H": 9},
        {"TH9H": 1, "QH6H": 3},
        {"3H2S": 4, "KD7S": 8}]),
    # flop, 6 seats: 0, 2 and 5 hold a known hand, the others 4 hands each
    "L5": _case("3S 8S KS", [
        {"8H7S": 4},
        {"QH7D": 9, "KC7H": 3, "8C2H": 1, "AC2C": 9},
        {"KHKD": 1},
        {"8H8C": 6, "AC2C": 7, "2S2D": 8, "KD7D": 3},
        {"AHAD": 5, "AS8D": 3, "QS3H": 3, "3D3C": 8},
        {"QDQC": 1}]),
    # before the flop, 3 seats, 2 hands each: broadway cards that get in each other's way, suited or not, and a pair of aces
    "L6": _case("", [
        {"ASQC": 4, "KSJD": 6},
        {"ASJH": 4, "KDQD": 8},
        {"KCJC": 1, "AHAC": 4}]),
    # flop, two known hands and one seat with weight 65535 on all 1326 hands: one uniform random opponent, and the only
    # cases with the table total at its maximum, 1326 * 65535 = 86 899 410
    "L7": _case("TS JS QD", [{"ACKH": 3}, wide(65535), {"AS9C": 8}]),
    "L8": _case("2H 9H TC", [
        {"QSTH": 3}, {"3C2C": 8}, {"9S8D": 7}, {"AD8S": 8}, wide(65535),
        {"KD6H": 1}, {"QH4D": 8}, {"5S3D": 4}, {"4C2D": 7}, {"TS6C": 4}]),
    # turn, 6 seats, every seat a known hand: no trial is ever abandoned
    "H6": _case("6C 7D 8H KS", [{"ACKC": 3}, {"5D5C": 8}, {"9S9D": 7}, {"AS9H": 8}, {"AD6H": 1}, {"KD5S": 8}]),
}
HOST_CASES = ("L1", "L2", "H6")   # at most one table card to come: the literal enumeration is cheap
