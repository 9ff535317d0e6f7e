"""The evaluator's hand-type families, shape by shape, on the host build of the kernels' source (tests/hostsim).

mcq_eval_key decides nothing by a branch: quads ride on the straight lookup, two pairs and full houses share one
compare between two table entries, and a family that does not apply leaves a number that must stay below the hand's
true key.  Random hands reach most of these shapes rarely (quads: 0.17 %), so every shape is enumerated here over all
ranks -- suits and the position of the two hole cards by a fixed seeded sample -- and scored by the oracle's port of
hand_evaluator._calc_score.  Category AND total order must agree, the latter over all hands of this file together with
the 50 000 reference-scored hands of tests/golden/evaluator_hands.npz."""
import itertools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim as H

G = os.path.join(os.path.dirname(__file__), "golden")
SUIT_SAMPLES = 3  # per rank pattern: suits and hole position redrawn this often


def _deal(g, counts):
    """7 distinct card ids (rank * 4 + suit) holding counts[r] cards of rank r, in a random order (= random hole cards)."""
    hand = []
    for r, n in counts.items():
        hand += [4 * r + int(s) for s in g.permutation(4)[:n]]
    assert len(hand) == 7 and len(set(hand)) == 7
    return [int(c) for c in g.permutation(hand)]


def _rank_patterns(pattern, free=tuple(range(13))):
    """Every assignment of distinct ranks to `pattern` (multiplicities, e.g. (4, 2, 1), equal ones adjacent); ranks of
    equal multiplicity are an unordered choice."""
    if not pattern:
        yield ()
        return
    k = sum(1 for m in pattern if m == pattern[0])
    for head in itertools.combinations(free, k):
        rest = tuple(r for r in free if r not in head)
        for tail in _rank_patterns(pattern[k:], rest):
            yield head + tail


def _shape(g, pattern):
    hands = []
    for ranks in _rank_patterns(pattern):
        for _ in range(SUIT_SAMPLES):
            hands.append(_deal(g, dict(zip(ranks, pattern))))
    return hands


SHAPES = {
    # (a) four of a kind with every shape of the other three cards; ranks above and below the quads included
    "quads+trips": ((4, 3), 13 * 12),
    "quads+pair+kicker": ((4, 2, 1), 13 * 12 * 11),
    "quads+three kickers": ((4, 1, 1, 1), 13 * 220),
    # (b) the two-pair / full-house family and the hands it must stay out of
    "two trips": ((3, 3, 1), 78 * 11),
    "trips+two pairs": ((3, 2, 2), 13 * 66),
    "trips+pair+two kickers": ((3, 2, 1, 1), 13 * 12 * 55),
    "trips alone": ((3, 1, 1, 1, 1), 13 * 495),
    "three pairs": ((2, 2, 2, 1), 286 * 10),
    "two pairs": ((2, 2, 1, 1, 1), 78 * 165),
    "one pair": ((2, 1, 1, 1, 1, 1), 13 * 792),
    "no pair": ((1,) * 7, 1716),
}


def _score(hands):
    out = []
    for h in hands:
        _, ranks, typ = O.calc_score(h)
        out.append((typ, ranks))
    return out


@pytest.fixture(scope="module")
def scored():
    """{shape: (hands [n, 7], keys [n], reference tuples)}; the seed is per shape, so a shape's hands do not depend on
    which other shapes ran."""
    out = {}
    for i, (name, (pattern, n_patterns)) in enumerate(SHAPES.items()):
        hands = _shape(np.random.default_rng(1000 + i), pattern)
        assert len(hands) == n_patterns * SUIT_SAMPLES, name  # no rank pattern skipped
        hands = np.array(hands, np.uint8)
        out[name] = (hands, H.eval7(hands), _score(hands))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_category_of_every_shape(scored, name):
    hands, keys, ref = scored[name]
    cat = H.key_type(keys)
    for i in range(len(hands)):
        assert int(cat[i]) == ref[i][0], (name, hands[i], hex(int(keys[i])), ref[i])
    if name.startswith("quads"):
        assert all(O.TYPES[t] == "FoufOfAKind" for t, _ in ref)
        # the reference's quirk: the two highest DISTINCT ranks of all seven cards, not quad rank + kicker
        for i in range(len(hands)):
            top2 = tuple(sorted({int(c) >> 2 for c in hands[i]}, reverse=True)[:2])
            assert ref[i][1] == top2, (hands[i], ref[i])


def _check_total_order(keys, tup, what):
    order = np.argsort(keys, kind="stable")
    for a, b in zip(order[:-1], order[1:]):  # neighbours in key order: the strongest test of a total order
        if keys[a] == keys[b]:
            assert tup[a] == tup[b], (what[a], what[b], tup[a], tup[b])
        else:
            assert tup[a] < tup[b], (what[a], what[b], tup[a], tup[b])


@pytest.mark.parametrize("name", list(SHAPES))
def test_order_within_every_shape(scored, name):
    hands, keys, ref = scored[name]
    _check_total_order(keys, ref, hands)


def test_fixture_hands_category_and_order():
    z = np.load(os.path.join(G, "evaluator_hands.npz"))
    cards, cat, nr, ranks = z["cards"], z["category"], z["n_ranks"], z["card_ranks"]
    assert len(cards) == 50000
    keys = H.eval7(cards)
    assert np.array_equal(H.key_type(keys), cat)
    tup = [(int(cat[i]), tuple(int(x) for x in ranks[i, :nr[i]])) for i in range(len(cards))]
    _check_total_order(keys, tup, cards)


def test_one_total_order_over_all_shapes_and_the_fixture(scored):
    z = np.load(os.path.join(G, "evaluator_hands.npz"))
    cards, cat, nr, ranks = z["cards"], z["category"], z["n_ranks"], z["card_ranks"]
    hands = [cards]
    keys = [H.eval7(cards)]
    tup = [(int(cat[i]), tuple(int(x) for x in ranks[i, :nr[i]])) for i in range(len(cards))]
    for name in SHAPES:
        h, k, r = scored[name]
        hands.append(h)
        keys.append(k)
        tup += r
    hands, keys = np.concatenate(hands), np.concatenate(keys)
    assert len(hands) == len(tup) == 50000 + SUIT_SAMPLES * sum(n for _, n in SHAPES.values())
    _check_total_order(keys, tup, hands)
    # and the oracle scores the fixture's hands as the reference did (the two sources of expected values agree)
    g = np.random.default_rng(7)
    for i in g.choice(50000, 2000, replace=False):
        assert _score([cards[i]])[0] == tup[i], cards[i]
