"""Test helper: the cases of the hero-range exact enumeration (mcq_exact_batch_hero_range) and an independent ground truth.

A case is (hero range, opponent range, table cards, ghost cards); a range is a set of class strings, a top fraction of the
169 classes, or None for every class.  records(case) builds its (mcq_query, mcq_query_ext) pair; hand_records(case, hands)
the one-record form -- hero given as two cards -- of each hand, what mcq_exact_batch_ext enumerates.

literal(case, uniform) walks tools/montecarlo_python.py:121-189 as tests/exact_literal.py does, with the hero drawn first
as the law draws a ranged hand (:136-148: every accepted ORDERED index pair r1 in range(L), r2 in range(L - 1), r1 != r2
whose class is allowed; the hand deck[r1], deck[r2] leaves by value), then the opponent, then the table; everything in
fractions.Fraction.
"""
from fractions import Fraction

import numpy as np

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import exact_literal as EL

C = npa.card_id
AS = 51

# name -> (hero range, opponent range, table, ghost)
CASES = {
    # 47 cards left, 1081 hero hands: the second thread group works; AS is in the deck (the hands holding the top card)
    "river_all": (None, None, ["3C", "6D", "7H", "TS", "KC"], None),
    # AS on the table: the deck's top card is AH; ghost cards; 42 opponent classes
    "turn_ghost": (0.10, 0.25, ["AS", "9D", "4H", "QC"], ["2C", "KD"]),
    "flop_3cls": ({"AKS", "QQ", "T9O"}, 0.25, ["2D", "9H", "JS"], None),
    # AS among the ghost cards; a hero range one class wide
    "turn_one_class": ({"77"}, None, ["7C", "8D", "KH", "2S"], ["AS", "5C"]),
    "river_small": ({"AKS", "QQ", "T9O", "72O"}, 0.25, ["3C", "6D", "7H", "TS", "KC"], None),
    "turn_small": ({"QQ", "AKS"}, {"AA", "KK", "QQ", "AKS", "AKO", "JTS", "98S", "T9O", "76S", "KQO", "55", "A5S"},
                   ["QD", "9S", "4H", "AC"], None),
    "flop_all": (None, None, ["2D", "9H", "JS"], None),
    "flop_top25": (0.25, 0.25, ["5C", "8D", "QH"], None),
    "turn_vs_any": (0.25, None, ["5C", "8D", "QH", "KS"], None),
}
HOST_CASES = ["river_all", "turn_ghost", "flop_3cls", "turn_one_class"]
UNDEALABLE = ({"AA"}, {"AA"}, ["AD", "AC", "7H"], None)


def bits(rng):
    """A range -> its 6-word set, None for every class."""
    return mh._opponent_range_bits(1 if rng is None else rng)


def parts(case):
    hero, opp, table, ghost = case
    return bits(hero), bits(opp), [C(c) for c in table], None if ghost is None else [C(c) for c in ghost]


def records(case, n_players=2, hero_is_range=True):
    hb, ob, table, ghost = parts(case)
    q = _lib.pack_query_one([0, 0], table, n_players, 1)
    x = _lib.pack_query_ext(1, ghost=ghost, hero_range=(_lib.ALL_CLASSES if hb is None else hb) if hero_is_range else None,
                            opp_range=ob)
    return q, x


def batch(cases):
    qs, xs = zip(*[records(c) for c in cases])
    return np.concatenate(qs), np.concatenate(xs)


def deck(case):
    _, _, table, ghost = parts(case)
    return [c for c in range(52) if c not in table and c not in (ghost or [])]


def allowed_hands(case):
    """The hands {a < b} of the deck whose class is in the hero's range, in ascending row order."""
    hb = EL.bits_to_set(parts(case)[0])
    d = deck(case)
    out = [(a, b) for b in d for a in d if a < b and (hb is None or EL.class_bit(a, b) in hb)]
    return sorted(out, key=lambda h: _lib.hand_index(*h))


def hand_records(case, hands):
    """The one-record form of every hand: hero given as two cards, one opponent from the same range."""
    _, ob, table, ghost = parts(case)
    q = np.concatenate([_lib.pack_query_one(list(h), table, 2, 1) for h in hands])
    x = _lib.pack_query_ext(len(hands), ghost=ghost, opp_range=ob)
    return q, x


def hero_draw(case, uniform):
    """-> {hand (a < b): how many accepted draws deal it}: the literal index walk of montecarlo_python.py:136-148."""
    hb = EL.bits_to_set(parts(case)[0])
    d = deck(case)
    ok = (lambda a, b: True) if hb is None else (lambda a, b: EL.class_bit(a, b) in hb)
    w = {}
    if uniform:
        return {h: 1 for h in allowed_hands(case)}
    L = len(d)
    for r1 in range(L):
        for r2 in range(L - 1):
            if r1 != r2 and ok(d[r1], d[r2]):
                h = tuple(sorted((d[r1], d[r2])))
                w[h] = w.get(h, 0) + 1
    return w


def literal(case, uniform):
    """-> ({hand: [win, tie, by_type[9]] as Fractions}, the aggregate's eleven Fractions)."""
    _, ob, table, _ = parts(case)
    opp = EL.bits_to_set(ob)
    k = 5 - len(table)
    score = EL._Scores()
    draw = hero_draw(case, uniform)
    total = sum(draw.values())
    per, agg = {}, [Fraction(0)] * 11
    for h, cnt in draw.items():
        d1 = [c for c in deck(case) if c not in h]
        w1, n1 = EL._opponent(d1, opp, uniform)
        assert n1 > 0
        acc = [Fraction(0)] * 11
        for g, a in w1.items():
            tabs, tot = EL._tables([c for c in d1 if c not in g], k, uniform)
            s = [0] * 11
            for t, wt in tabs.items():
                full = tuple(table) + t
                hs, htype = score(h, full)
                gs = score(g, full)[0]
                if hs > gs:
                    s[0] += wt
                    s[2 + htype] += wt
                elif hs == gs:
                    s[1] += wt
                    s[2 + htype] += wt
            for i in range(11):
                acc[i] += Fraction(a, n1) * Fraction(s[i], tot)
        per[h] = acc
        for i in range(11):
            agg[i] += Fraction(cnt, total) * acc[i]
    return per, agg


def row_fractions(row13):
    """A 13-word weights row -> its eleven probabilities as Fractions."""
    r = [int(v) for v in row13]
    return [Fraction(r[2], r[0]), Fraction(r[3], r[0])] + [Fraction(v, r[0]) for v in r[4:13]]
