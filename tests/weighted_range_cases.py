"""Test helper: the cases of the WEIGHTED hero-range exact enumeration (mcq_exact_batch_hero_range_weighted) and an
independent ground truth.

A case is a tests/hero_range_cases.py case (hero classes, opponent classes, table cards, ghost cards) with two weight
tables beside it: opp[1326] and hero[1326] (or None) of uint16, indexed by hand_index(a, b).  The class sets stay in
force: a hand's effective weight is its table entry if its class is in the set, else 0.

literal(case, opp, hero) walks the definition directly: for every allowed hero hand h, every k-subset T of D minus h and
every hand g of D minus h minus T, the weight eff_opp(g) goes to win / tie / runs by the comparison of the two hands'
scores.  The scores are the oracle's evaluator (what tests/exact_literal.py scores with, here through its batch entry:
one order-preserving integer per seven cards); none of the library's lane code is involved.  The sums are exact integers
and the aggregate is combined in fractions.Fraction.
"""
from fractions import Fraction
from itertools import combinations

import numpy as np

from neuron_poker_amd import _lib
from oracle import oracle as O
from tests import exact_literal as EL
from tests import hero_range_cases as HC

ROWS = 1326
WMAX = 65535
HANDS = [(a, b) for b in range(52) for a in range(b)]            # row hand_index(a, b) -> (a, b)
CLASS_OF = np.array([EL.class_bit(a, b) for a, b in HANDS])      # row -> class bit


def ones():
    return np.ones(ROWS, np.uint16)


def all_max():
    return np.full(ROWS, WMAX, np.uint16)


def class_aligned(seed):
    """One value from {0, 1, 3, 1000} per preflop class."""
    v = np.random.default_rng(seed).choice(np.array([0, 1, 3, 1000], np.uint16), 169)
    return v[CLASS_OF].astype(np.uint16)


def hand_level(seed):
    """Suit-specific: every hand its own weight -- a third of them 0, the others anywhere in 1..65535, small values and
    the largest one among them."""
    g = np.random.default_rng(seed)
    kind = g.integers(0, 6, ROWS)
    w = np.where(kind < 2, 0, np.where(kind == 2, g.integers(1, 8, ROWS), np.where(kind == 3, WMAX, g.integers(1, WMAX + 1, ROWS))))
    return w.astype(np.uint16)


def hero_table(seed):
    """A hero table with zeros inside allowed classes: half of the hands 0, the others 1, 7 or 40000."""
    g = np.random.default_rng(seed)
    return g.choice(np.array([0, 0, 0, 1, 7, 40000], np.uint16), ROWS).astype(np.uint16)


def split_classes(w):
    """The class bits of which `w` gives some hands 0 and some not."""
    return [c for c in range(169) if (w[CLASS_OF == c] == 0).any() and (w[CLASS_OF == c] != 0).any()]


# name -> (case of tests/hero_range_cases.py, opponent table, hero table or None)
WCASES = {
    "river_hand_level": ("river_all", hand_level(11), None),
    "turn_ghost_class": ("turn_ghost", class_aligned(12), None),
    "flop_3cls_hero": ("flop_3cls", hand_level(13), hero_table(14)),
    "flop_all_hand_level": ("flop_all", hand_level(15), None),
    "flop_all_max": ("flop_all", all_max(), None),
    "flop_top25_class": ("flop_top25", class_aligned(16), None),
    "turn_hero_zeros": ("turn_vs_any", hand_level(17), hero_table(18)),
}
assert split_classes(WCASES["river_hand_level"][1]) and not split_classes(class_aligned(12))
for _w in WCASES.values():
    for _t in _w[1:]:
        if _t is not None:
            _t.setflags(write=False)


def records(name):
    """-> (mcq_query, mcq_query_ext, opp[1, 1326], hero[1, 1326] or None) of a weighted case."""
    base, opp, hero = WCASES[name]
    q, x = HC.records(HC.CASES[base])
    return q, x, opp.reshape(1, ROWS), None if hero is None else hero.reshape(1, ROWS)


def batch(names):
    """One batch of weighted cases; a missing hero table becomes its definition, every entry 1."""
    recs = [records(n) for n in names]
    return (np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs]), np.concatenate([r[2] for r in recs]),
            np.concatenate([ones().reshape(1, ROWS) if r[3] is None else r[3] for r in recs]))


def effective(case, opp, hero):
    """-> (eff_opp[1326], eff_hero[1326]) as Python-int arrays: the tables with the class sets and the deck folded in
    (0 for a hand that holds a table or ghost card)."""
    hb, ob, _, _ = HC.parts(case)
    hs, os_ = EL.bits_to_set(hb), EL.bits_to_set(ob)
    d = set(HC.deck(case))
    in_deck = np.array([a in d and b in d for a, b in HANDS])
    in_h = np.array([hs is None or c in hs for c in CLASS_OF])
    in_o = np.array([os_ is None or c in os_ for c in CLASS_OF])
    h = np.ones(ROWS, np.int64) if hero is None else np.asarray(hero).reshape(ROWS).astype(np.int64)
    o = np.asarray(opp).reshape(ROWS).astype(np.int64)
    return np.where(in_deck & in_o, o, 0), np.where(in_deck & in_h, h, 0)


def literal(case, opp, hero, only=None):
    """-> ({hand: [runs, win, tie, by_type[9]] as Python ints}, the aggregate's eleven Fractions).  only: walk just these
    hero hands (the aggregate is then theirs)."""
    _, _, table, _ = HC.parts(case)
    eff_o, eff_h = effective(case, opp, hero)
    d = HC.deck(case)
    k = 5 - len(table)
    allowed = [h for h in combinations(d, 2) if eff_h[_lib.hand_index(*h)] > 0]
    if only is not None:
        allowed = [h for h in allowed if h in only]
    sums = {h: [0] * 12 for h in allowed}
    for T in combinations(d, k):
        rest = [c for c in d if c not in T]
        g = np.array(list(combinations(rest, 2)), np.int64)                 # every hand of D minus T
        seven = np.concatenate([g, np.tile(np.array(table + list(T), np.int64), (len(g), 1))], axis=1)
        score = O.score_batch(seven.astype(np.uint8))
        wt = eff_o[g[:, 1] * (g[:, 1] - 1) // 2 + g[:, 0]]
        where = {(int(a), int(b)): i for i, (a, b) in enumerate(g)}
        for h in allowed:
            i = where.get(h)
            if i is None:
                continue                                                    # h holds a card of T
            free = (g[:, 0] != h[0]) & (g[:, 0] != h[1]) & (g[:, 1] != h[0]) & (g[:, 1] != h[1])
            w = np.where(free, wt, 0)
            win, tie = int(w[score < score[i]].sum()), int(w[score == score[i]].sum())
            s = sums[h]
            s[0] += int(w.sum())
            s[1] += win
            s[2] += tie
            s[3 + int(score[i] >> np.uint64(32))] += win + tie
    agg, den = [Fraction(0)] * 11, sum(int(eff_h[_lib.hand_index(*h)]) for h in allowed)
    for h in allowed:
        s, wh = sums[h], int(eff_h[_lib.hand_index(*h)])
        assert s[0] > 0, ("no opponent hand against", h)
        for i in range(11):
            agg[i] += Fraction(wh * s[1 + i], s[0] * den)
    return sums, agg


def row_ints(row13):
    """A 13-word row -> [runs, win, tie, by_type[9]] as Python ints (passes, word 1, must be 0)."""
    r = [int(v) for v in row13]
    assert r[1] == 0
    return [r[0]] + r[2:13]
