"""Test helper: a literal walk of small exact cases that records k, the number of hands sharing the pot.

In the style of tests/exact_literal.py (whose dealing helpers it reuses unchanged): the deck is a list in card-id order;
ghost, table, hero and the known hands leave it by value; one random opponent is every accepted index pair under the
reference's law, or every allowed unordered hand under the uniform law; then every table completion.  Everything in
fractions.Fraction, outcome by outcome.  Small cases only (river and turn boards)."""
from fractions import Fraction

from tests.exact_literal import _Scores, _opponent, _tables, bits_to_set


def exact_ways(hero, board, n_players, known=(), ghost=None, opp_range=None, uniform=False):
    """-> (win, tie_by_k) as Fractions: tie_by_k[k - 2] = P(hero is best together with k - 1 other hands), k = 2..10."""
    allowed = bits_to_set(opp_range)
    deck = list(range(52))
    for c in list(ghost or []) + list(board) + list(hero) + [c for h in known for c in h]:
        deck.remove(c)
    n_r = n_players - 1 - len(known)
    assert 0 <= n_r <= 1
    k = 5 - len(board)
    score = _Scores()
    hero = tuple(sorted(hero))
    known = [tuple(sorted(h)) for h in known]
    win, ties = [Fraction(0)], [Fraction(0)] * 9

    def showdown(opps, deck_after, weight):
        tabs, tot = _tables(deck_after, k, uniform)
        for t, wt in tabs.items():
            table = tuple(board) + t
            hs = score(hero, table)[0]
            others = [score(h, table)[0] for h in known + list(opps)]
            if any(o > hs for o in others):
                continue
            n_eq = sum(1 for o in others if o == hs)
            p = weight * Fraction(wt, tot)
            if n_eq == 0:
                win[0] += p
            else:
                ties[n_eq - 1] += p

    if n_r == 0:
        showdown((), deck, Fraction(1))
    else:
        w1, n1 = _opponent(deck, allowed, uniform)
        assert n1 > 0, "range cannot be dealt"
        for h1, a in w1.items():
            showdown((h1,), [c for c in deck if c not in h1], Fraction(a, n1))
    return win[0], ties
