"""Expectations shared by the per-seat tests (host and GPU): mcq_result_seats rows as 32 words -- runs, passes, then win,
tie, share of seat 0..9.

recount() recounts every seat from the hands the host build of the lane code dealt, with the oracle's own comparison;
exact_seats_literal() is an independent per-seat walk of the all-in case in fractions, built from the pieces of
tests/exact_literal.py (river, turn and flop boards: a preflop walk is 1.7 million completions)."""
from fractions import Fraction

import numpy as np

import neuron_poker_amd as npa
from oracle import oracle as O
from tests.exact_literal import _Scores, _tables, bits_to_set  # noqa: F401  (bits_to_set: the callers' range helper)

UNIT = 2520
WORDS = 32


def seat_words(row):
    """[10, 3] view (win, tie, share) of a 32-word row."""
    return np.asarray(row, np.uint64).reshape(WORDS)[2:].reshape(10, 3)


def recount(hands, n_players, ks=None):
    """[10, 3] uint64 win, tie, share per seat, recounted from the dealt hands [runs, 2 n + 5] with oracle.compare: per
    iteration the best of ALL hands and every seat level with it (not hero against the rest).  ks (a set, optional)
    collects the numbers of hands that shared a pot."""
    out = np.zeros((10, 3), np.uint64)
    for row in hands:
        table = [int(c) for c in row[2 * n_players:]]
        seven = [[int(row[2 * p]), int(row[2 * p + 1])] + table for p in range(n_players)]
        level = [0]
        for p in range(1, n_players):
            c = O.compare(seven[p], seven[level[0]])   # > 0: hand p is greater
            if c > 0:
                level = [p]
            elif c == 0:
                level.append(p)
        k = len(level)
        if ks is not None:
            ks.add(k)
        for p in level:
            out[p, 0 if k == 1 else 1] += 1
            out[p, 2] += UNIT // k
    return out


def hero_share_from_ways(ways_row):
    """seat[0].share of the per-seat row from the 22-word split-pot row of the same query."""
    w = [int(x) for x in np.asarray(ways_row).view(np.uint64).reshape(22)]
    return UNIT * w[2] + sum((UNIT // k) * w[13 + k - 2] for k in range(2, 11))


def check_invariants(row, n_players):
    r = [int(x) for x in np.asarray(row).view(np.uint64).reshape(WORDS)]
    runs, seats = r[0], seat_words(row).astype(object)
    assert sum(int(s[2]) for s in seats) == UNIT * runs, (r, n_players)
    assert sum(int(s[0]) for s in seats) <= runs
    assert all(int(s[0]) + int(s[1]) <= runs for s in seats)
    assert not any(int(x) for s in seats[n_players:] for x in s)


_host = {}


def host_row(i, runs, seed, qid):
    """The host lane build's 32-word row of ext_ways_cases.CASES[i] (cached: computed once, shared by the tests)."""
    from tests import ext_ways_cases as XC
    from tests import hostsim_seats as H
    key = (i, runs, seed, qid)
    if key not in _host:
        q, ext = XC.records(XC.CASES[i], runs)
        _host[key] = H.run(q, ext, seed, qid)
    return _host[key]


def exact_seats_literal(hands, board, ghost=None, uniform=False):
    """The all-in case, seat by seat: -> [(P(win), P(tie), pot share)] as Fractions, one per hand.  Cards as ids; hands[0]
    is the hero.  The deck is what tools/montecarlo_python.py leaves (ghost, table and every hand gone by value); the table
    completions and their weights come from tests.exact_literal._tables (the reference never deals the deck's last card)."""
    deck = list(range(52))
    for c in list(ghost or []) + list(board) + [c for h in hands for c in h]:
        deck.remove(c)
    score = _Scores()
    hands = [tuple(sorted(h)) for h in hands]
    tabs, tot = _tables(deck, 5 - len(board), uniform)
    acc = [[0, 0, Fraction(0)] for _ in hands]
    for t, wt in tabs.items():
        table = tuple(board) + t
        s = [score(h, table)[0] for h in hands]
        best = max(s)
        level = [i for i, x in enumerate(s) if x == best]
        for i in level:
            acc[i][0 if len(level) == 1 else 1] += wt
            acc[i][2] += Fraction(wt, len(level))
    return [(Fraction(a[0], tot), Fraction(a[1], tot), a[2] / tot) for a in acc]


def ids(cards):
    return [npa.card_id(c) for c in cards]


# the all-in cases of the exact tests: (hands, board, ghost).  2, 3, 6 and 10 hands; river, turn and one flop board.
EXACT_SMALL = [
    ([["AH", "KD"], ["QS", "QC"]], ["2C", "7D", "9H", "JS", "3S"], None),
    ([["AH", "KD"], ["QS", "QC"]], ["2C", "7D", "9H", "JS"], ["AS", "AD"]),
    ([["AH", "KD"], ["AS", "KC"], ["AD", "KH"]], ["2H", "7H", "9C"], None),               # three level hands, two flush draws
    ([["AH", "KD"], ["AS", "KC"], ["QS", "QC"]], ["2C", "7D", "9H", "JS"], ["AD", "KH"]),
    ([["2C", "3D"], ["4H", "5D"], ["9C", "9D"], ["AH", "AD"], ["7C", "8D"], ["6H", "6D"]], ["KC", "KD", "KH", "KS"], None),
    # the board plays for everybody: a ten-way split
    ([["2C", "3D"], ["2D", "3C"], ["2H", "3H"], ["4C", "5D"], ["4D", "5C"], ["4H", "5H"], ["6C", "7D"], ["6D", "7C"],
      ["6H", "7H"], ["8C", "9D"]], ["TS", "JS", "QS", "KS", "AS"], None),
    ([["AH", "KD"], ["AS", "KC"], ["AD", "KH"], ["2C", "2D"], ["3C", "3D"], ["4C", "4D"], ["5C", "5D"], ["6C", "6D"],
      ["7C", "7D"], ["8C", "8D"]], ["9H", "TH", "JS", "QS"], None),
]


def exact_records(case):
    """-> (mcq_query record [1], mcq_query_ext record [1]) of an all-in case."""
    hands, board, ghost = case
    b = ids(board)
    q = npa.pack_queries([ids(hands[0])], [b + [255] * (5 - len(b))], len(hands), 1)
    ext = npa.pack_query_ext(1, ghost=ids(ghost) if ghost else None, known=[ids(h) for h in hands[1:]])
    return q, ext


def assert_exact_row(row, case, law):
    """A 32-word weight row against the literal walk."""
    hands, board, ghost = case
    lit = exact_seats_literal([ids(h) for h in hands], ids(board), ids(ghost) if ghost else None, uniform=bool(law))
    r = [int(x) for x in np.asarray(row).view(np.uint64).reshape(WORDS)]
    tot = r[0]
    assert tot > 0 and r[1] == 0
    for s, (win, tie, share) in enumerate(lit):
        assert Fraction(r[2 + 3 * s], tot) == win, (s, case)
        assert Fraction(r[3 + 3 * s], tot) == tie, (s, case)
        assert Fraction(r[4 + 3 * s], UNIT * tot) == share, (s, case)
    check_invariants(row, len(hands))
