"""Test helper: the cases of the per-runout exact enumeration (mcq_exact_batch_ext_runouts) and an independent ground truth.

literal(case, uniform) is the index-by-index walk of tools/montecarlo_python.py:121-189 in the style of
tests/exact_literal.py (whose dealing helpers and scores it reuses unchanged): the deck is a list in card-id order; ghost,
table, hero and the known hands leave it by value; one random opponent is every accepted index pair under the reference's
law, or every allowed unordered hand under the uniform law; then the new table cards one after the other, deck.pop(i) for
i in range(len(deck) - 1) (every index under the uniform law).  Per COMPLETION (the sorted new cards) it keeps, in
fractions.Fraction, the probability of the completion together with a win, a tie, a tie shared k ways and hero's hand
type.  The walk of the table cards is ORDERED, so it also gives P(first new card = c) without any symmetry argument.
Small cases only."""
from fractions import Fraction

import numpy as np

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from tests.exact_literal import _Scores, _opponent, bits_to_set

C = npa.card_id

# name -> (hero, table, n_players, known hands, ghost, opponent range: a set of class strings or None for every class)
CASES = {
    # (a) turn, heads-up against a 3-class range
    "turn_3cls": (["AH", "KH"], ["QH", "JD", "2C", "7S"], 2, [], None, {"QQ", "AKO", "T9S"}),
    # (b) turn, a known hand, a ranged opponent and ghost cards; AS is a ghost card: the deck's top card is AH
    "turn_known_ghost": (["KH", "QH"], ["JH", "9S", "4D", "4C"], 3, [["9C", "9D"]], ["AS", "5C"], {"JJ", "A4S", "KQO"}),
    # (c) flop all-in, three known hands (no random opponent: a lane per completion, k = 2); a shared straight ties three ways
    "flop_allin": (["AC", "KD"], ["QS", "JH", "TC"], 4, [["AD", "KS"], ["AH", "2C"], ["9D", "9H"]], None, None),
    # (d) flop against a 3-class range
    "flop_3cls": (["TS", "9S"], ["8S", "7D", "2H"], 2, [], None, {"88", "A8O", "JTS"}),
    # (e) flop against any hand, hero only: 47 cards, 1081 completions
    "flop_any": (["AS", "KS"], ["QS", "7D", "2H"], 2, [], None, None),
    # hero alone on a flop: the all-in shape with more completions (1081) than a block has lanes
    "flop_alone": (["AS", "KS"], ["QS", "7D", "2H"], 1, [], None, None),
    # GPU batch only: a turn all-in and a flop with a known hand and an unrestricted opponent
    "turn_allin": (["AC", "KD"], ["QS", "JH", "3C", "3D"], 3, [["AD", "KS"], ["3H", "8C"]], None, None),
    "flop_known_any": (["7C", "7D"], ["AH", "8S", "2D"], 3, [["AC", "QD"]], ["KS", "KH"], None),
}
LITERAL_CASES = ["turn_3cls", "turn_known_ghost", "flop_allin", "flop_3cls"]
HOST_CASES = LITERAL_CASES + ["flop_any", "flop_alone"]
GPU_CASES = HOST_CASES + ["turn_allin", "flop_known_any"]


def parts(case):
    hero, table, n_players, known, ghost, opp = case
    return ([C(c) for c in hero], [C(c) for c in table], n_players, [[C(c) for c in h] for h in known],
            None if ghost is None else [C(c) for c in ghost], None if opp is None else _lib.range_bits(opp))


def records(case):
    hero, table, n_players, known, ghost, opp = parts(case)
    return _lib.pack_query_one(hero, table, n_players, 1), _lib.pack_query_ext(1, ghost=ghost, known=known, opp_range=opp)


def batch(names):
    qs, xs = zip(*[records(CASES[n]) for n in names])
    return np.concatenate(qs), np.concatenate(xs)


def deck(case):
    """R: the cards the opponent and the table are dealt from, ascending."""
    hero, table, _, known, ghost, _ = parts(case)
    gone = set(hero) | set(table) | set(ghost or []) | {c for h in known for c in h}
    return [c for c in range(52) if c not in gone]


class Outcome:
    """What one completion adds: probabilities of the completion (p), with a win, with a tie, with a tie shared by
    k = 2..10 hands; hero's hand type there."""

    def __init__(self, htype):
        self.p, self.win, self.tie, self.ways, self.type = Fraction(0), Fraction(0), Fraction(0), [Fraction(0)] * 9, htype


def literal(case, uniform):
    """-> ({completion (sorted card ids): Outcome}, {card: P(it is the first new table card)})."""
    hero, table, n_players, known, _, opp = parts(case)
    allowed = bits_to_set(opp)
    d0 = deck(case)
    n_r = n_players - 1 - len(known)
    assert 0 <= n_r <= 1
    k = 5 - len(table)
    assert k in (1, 2)
    score = _Scores()
    hero = tuple(sorted(hero))
    known = [tuple(sorted(h)) for h in known]
    per, first = {}, {}

    def showdown(opps, d, weight):
        n1 = len(d) if uniform else len(d) - 1
        for i in range(n1):
            c1 = d[i]
            d2 = d[:i] + d[i + 1:]
            n2 = 1 if k == 1 else (len(d2) if uniform else len(d2) - 1)
            first[c1] = first.get(c1, Fraction(0)) + weight * Fraction(1, n1)
            for j in range(n2):
                t = (c1,) if k == 1 else tuple(sorted((c1, d2[j])))
                p = weight * Fraction(1, n1 * n2)
                full = tuple(table) + t
                hs, htype = score(hero, full)
                o = per.get(t)
                if o is None:
                    o = per[t] = Outcome(htype)
                assert o.type == htype
                o.p += p
                others = [score(h, full)[0] for h in known + list(opps)]
                if any(s > hs for s in others):
                    continue
                n_eq = sum(1 for s in others if s == hs)
                if n_eq == 0:
                    o.win += p
                else:
                    o.tie += p
                    o.ways[n_eq - 1] += p

    if n_r == 0:
        showdown((), d0, Fraction(1))
    else:
        w1, total = _opponent(d0, allowed, uniform)
        assert total > 0, "range cannot be dealt"
        for h1, a in w1.items():
            showdown((h1,), [c for c in d0 if c not in h1], Fraction(a, total))
    return per, first


def row_fractions(row22, total):
    """A 22-word weights row over the record's total weight -> (p, win, tie, by_type[9], ways[9]) as Fractions."""
    r = [int(v) for v in row22]
    assert r[1] == 0
    return (Fraction(r[0], total), Fraction(r[2], total), Fraction(r[3], total), [Fraction(v, total) for v in r[4:13]],
            [Fraction(v, total) for v in r[13:22]])


def outcome_fractions(o):
    """The same five of an Outcome (None: a completion that cannot come)."""
    if o is None:
        return Fraction(0), Fraction(0), Fraction(0), [Fraction(0)] * 9, [Fraction(0)] * 9
    return o.p, o.win, o.tie, [o.win + o.tie if t == o.type else Fraction(0) for t in range(9)], list(o.ways)
