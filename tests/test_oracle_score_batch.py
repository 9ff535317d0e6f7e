"""O.score_batch (mcqo_calc_score_batch: threaded, one order-preserving integer per hand) pinned where it is introduced:
it is O.calc_score packed the same way, on every reference-scored fixture hand and on every hand of the evaluator's
shape enumeration, and its integer order is O.compare's order."""
import os

import numpy as np

from oracle import oracle as O
from tests.test_eval_key_families_host import SHAPES, SUIT_SAMPLES, _shape

G = os.path.join(os.path.dirname(__file__), "golden")


def _packed_one_by_one(hands):
    out = np.zeros(len(hands), np.uint64)
    for i, h in enumerate(hands):
        _, ranks, typ = O.calc_score(h)
        out[i] = O.pack_score(typ, ranks)
    return out


def test_pack_score_is_python_tuple_order():
    tups = [(0, (12, 10, 5, 3, 1)), (0, (12, 10, 5, 3, 2)), (4, (3, 2, 1, 0, -1)), (4, (4, 3, 2, 1, 0)),
            (7, (12, 11)), (8, (3, 2, 1, 0)), (8, (3, 2, 1, 0, 0)), (8, (12, 3, 2, 1, 0, -1)), (8, (12, 11, 10, 9, 8, -1)),
            (8, (12, 11, 10, 9, 8, 3, 2, -1))]
    assert tups == sorted(tups)
    packed = [O.pack_score(*t) for t in tups]
    assert packed == sorted(packed) and len(set(packed)) == len(packed)
    assert O.pack_score(8, (12, 11, 10, 9, 8, 3, 2, -1)) == (8 << 32) | 0xDCBA9430


def test_fixture_hands_as_the_reference_scored_them():
    z = np.load(os.path.join(G, "evaluator_hands.npz"))
    cards, cat, nr, ranks = z["cards"], z["category"], z["n_ranks"], z["card_ranks"]
    assert len(cards) == 50000
    want = np.array([O.pack_score(int(cat[i]), [int(x) for x in ranks[i, :nr[i]]]) for i in range(len(cards))], np.uint64)
    assert int(nr.max()) == 8                                     # the longest tuple the packing must hold
    for threads in (1, 5, 16):
        assert np.array_equal(O.score_batch(cards, threads), want), threads
    assert np.array_equal(_packed_one_by_one(cards), want)
    assert np.array_equal(O.score_type(want), cat)


def test_every_hand_of_the_shape_enumeration():
    for i, (name, (pattern, n_patterns)) in enumerate(SHAPES.items()):
        hands = np.array(_shape(np.random.default_rng(1000 + i), pattern), np.uint8)   # the hands of that file's fixture
        assert len(hands) == n_patterns * SUIT_SAMPLES
        assert np.array_equal(O.score_batch(hands, 4), _packed_one_by_one(hands)), name


def test_integer_order_is_compare():
    z = np.load(os.path.join(G, "evaluator_hands.npz"))
    cards = z["cards"]
    s = O.score_batch(cards, 4)
    g = np.random.default_rng(20261)
    a, b = g.integers(0, len(cards), 20000), g.integers(0, len(cards), 20000)
    # ... and pairs that are close: neighbours in score order, where an order that is only nearly right would slip
    order = np.argsort(s, kind="stable")
    k = g.integers(0, len(cards) - 1, 20000)
    a, b = np.concatenate([a, order[k]]), np.concatenate([b, order[k + 1]])
    n_eq = 0
    for i, j in zip(a, b):
        c = O.compare(cards[i], cards[j])
        assert c == (int(s[i]) > int(s[j])) - (int(s[i]) < int(s[j])), (cards[i], cards[j], hex(int(s[i])), hex(int(s[j])))
        n_eq += c == 0
    assert 0 < n_eq < len(a)
