"""Test helper: an independent ground truth for the exact enumeration of extended queries.

It walks tools/montecarlo_python.py:121-189 index by index, as the reference executes it: the deck is a list in card-id
order; ghost cards, table cards and the known hands leave it by value; a random opponent is every accepted index pair
r1 in range(L), r2 in range(L - 1), r1 != r2, whose classes -- tested on the UNPOPPED deck[r1], deck[r2] -- are allowed,
then deck.pop(r1), deck.pop(r2); a table card is deck.pop(i) for i in range(len(deck) - 1).  Every stage is normalised
by its own count of accepted draws, in fractions.Fraction.  MCQ_LAW_UNIFORM is enumerated directly: every allowed
unordered hand still in the deck, then every table completion, equally likely.

Hands are scored by the oracle's evaluator (pinned to the reference's _calc_score), once per possible two-card hand and
completion; the walk compares those scores.  The hero wins ties, as eval_best_hand's stable sort credits them (the
reference's hand_evaluator.py:20-24).  Small cases only: a river with two ranged opponents is ~4e6 index pairs.
"""
from fractions import Fraction

from oracle import oracle as O


def class_bit(a, b):
    """Bit of two cards in a 169-bit range set (get_two_short_notation, montecarlo_python.py:24-34)."""
    ra, rb = a >> 2, b >> 2
    if ra == rb:
        return 14 * ra
    lo, hi = min(ra, rb), max(ra, rb)
    return 13 * lo + hi if (a & 3) == (b & 3) else 13 * hi + lo


def bits_to_set(words):
    """6-word range set -> set of class bits, None for every class."""
    if words is None:
        return None
    s = {i for i in range(169) if (int(words[i >> 5]) >> (i & 31)) & 1}
    return None if len(s) == 169 else s


class _Scores:
    """Score of (hand, completed table) -> comparable tuple, computed once."""

    def __init__(self):
        self.cache = {}

    def __call__(self, hand, table):
        key = (hand, table)
        s = self.cache.get(key)
        if s is None:
            score, ranks, t = O.calc_score(list(hand) + sorted(table))
            s = self.cache[key] = ((score, ranks, t), t)
        return s


def _opponent(deck, allowed, uniform):
    """-> ({hand (sorted pair): integer weight}, total) of one random opponent dealt from `deck` (a list)."""
    ok = (lambda a, b: True) if allowed is None else (lambda a, b: class_bit(a, b) in allowed)
    w = {}
    if uniform:
        for i in range(len(deck)):
            for j in range(i + 1, len(deck)):
                if ok(deck[i], deck[j]):
                    w[(deck[i], deck[j])] = 1
        return w, len(w)
    L = len(deck)
    total = 0
    for r1 in range(L):
        for r2 in range(L - 1):
            if r1 == r2 or not ok(deck[r1], deck[r2]):
                continue
            rest = deck[:r1] + deck[r1 + 1:]
            hand = tuple(sorted((deck[r1], rest[r2])))
            w[hand] = w.get(hand, 0) + 1
            total += 1
    return w, total


def _tables(deck, k, uniform):
    """-> ({completion (sorted tuple): integer weight}, total): k table cards from `deck`, one after the other."""
    out = {(): 1}
    for _ in range(k):
        nxt = {}
        for t, wt in out.items():
            d = [c for c in deck if c not in t]
            for i in range(len(d) if uniform else len(d) - 1):
                key = tuple(sorted(t + (d[i],)))
                nxt[key] = nxt.get(key, 0) + wt
        out = nxt
    return out, sum(out.values())


def exact(hero, board, n_players, known=(), ghost=None, opp_range=None, uniform=False):
    """Exact (win, tie, by_type[9]) as Fractions.  Cards as ids; opp_range = 6-word set or None."""
    allowed = bits_to_set(opp_range)
    deck = list(range(52))
    for c in list(ghost or []) + list(board) + list(hero) + [c for h in known for c in h]:
        deck.remove(c)
    n_r = n_players - 1 - len(known)
    assert 0 <= n_r <= 2
    k = 5 - len(board)
    score = _Scores()
    hero = tuple(sorted(hero))
    known = [tuple(sorted(h)) for h in known]
    acc = [Fraction(0)] * 11

    def showdown(opps, deck_after, weight):
        """All completions from deck_after; adds weight x P(completion) to the outcome of each."""
        tabs, tot = _tables(deck_after, k, uniform)
        s = [0] * 11
        for t, wt in tabs.items():
            table = tuple(board) + t
            hs, htype = score(hero, table)
            best = max([score(h, table)[0] for h in known + list(opps)], default=None)
            if best is None or hs > best:
                s[0] += wt
                s[2 + htype] += wt
            elif hs == best:
                s[1] += wt
                s[2 + htype] += wt
        for i in range(11):
            if s[i]:
                acc[i] += weight * Fraction(s[i], tot)

    if n_r == 0:
        showdown((), deck, Fraction(1))
    else:
        w1, n1 = _opponent(deck, allowed, uniform)
        assert n1 > 0, "range cannot be dealt"
        for h1, a in w1.items():
            d1 = [c for c in deck if c not in h1]
            if n_r == 1:
                showdown((h1,), d1, Fraction(a, n1))
                continue
            w2, n2 = _opponent(d1, allowed, uniform)
            assert n2 > 0, "range cannot be dealt"
            for h2, b in w2.items():
                d2 = [c for c in d1 if c not in h2]
                showdown((h1, h2), d2, Fraction(a, n1) * Fraction(b, n2))
    return acc
