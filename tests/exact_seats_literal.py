"""Test helper: a literal per-seat walk of small exact cases with at most one random opponent.

In the style of tests/exact_ways_literal.py, from the same pieces of tests/exact_literal.py (reused unchanged): the deck is
a list in card-id order; ghost, table, hero and the known hands leave it by value; the random opponent is every accepted
index pair under the reference's law, or every allowed unordered hand under the uniform law; then every table completion
from what is left.  Per outcome the best of ALL hands is found and every seat level with it is credited -- a win when it is
alone, a tie and 1/k of the pot when k seats are.  Everything in fractions.Fraction.  Small cases only (river and turn
boards).  Independent of the lane code: no candidate is sorted into above / level / below a known best here."""
from fractions import Fraction

from tests.exact_literal import _Scores, _opponent, _tables, bits_to_set


def exact_seats(hands, board, n_players, ghost=None, opp_range=None, uniform=False):
    """-> [(P(win), P(tie), pot share)] as Fractions, one per seat: hands[0] the hero, then the known hands, then (when
    n_players == len(hands) + 1) the random opponent.  Cards as ids; opp_range = 6-word set or None."""
    allowed = bits_to_set(opp_range)
    deck = list(range(52))
    for c in list(ghost or []) + list(board) + [c for h in hands for c in h]:
        deck.remove(c)
    n_r = n_players - len(hands)
    assert 0 <= n_r <= 1
    k = 5 - len(board)
    score = _Scores()
    hands = [tuple(sorted(h)) for h in hands]
    acc = [[Fraction(0), Fraction(0), Fraction(0)] for _ in range(n_players)]

    def showdown(opps, deck_after, weight):
        tabs, tot = _tables(deck_after, k, uniform)
        for t, wt in tabs.items():
            table = tuple(board) + t
            s = [score(h, table)[0] for h in hands + list(opps)]
            best = max(s)
            level = [i for i, x in enumerate(s) if x == best]
            p = weight * Fraction(wt, tot)
            for i in level:
                acc[i][0 if len(level) == 1 else 1] += p
                acc[i][2] += p / len(level)

    if n_r == 0:
        showdown((), deck, Fraction(1))
    else:
        w1, n1 = _opponent(deck, allowed, uniform)
        assert n1 > 0, "range cannot be dealt"
        for h1, a in w1.items():
            showdown((h1,), [c for c in deck if c not in h1], Fraction(a, n1))
    return [tuple(a) for a in acc]
