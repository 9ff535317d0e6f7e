"""The ranking key of seven cards over its WHOLE domain, on the host build of the kernels' source (tests/hostsim).

All C(52,7) = 133 784 560 hands, each under all 21 splits into (two hole cards, five table cards) -- 2.8e9 evaluations
of mcq_eval_key, nothing sampled -- against the oracle's restatement of hand_evaluator._calc_score
(O.score_batch: one order-preserving integer per hand):
  * the key does not depend on the split (the flush selector is made from the table cards, ge2/ge3/eq4 are composed from
    table and hole masks);
  * the key's type is the oracle's;
  * score -> key is strictly increasing on classes: equal scores have equal keys, and over all distinct (score, key)
    pairs both columns rise strictly together, so there are as many keys as scores (5034);
  * the census (hands and distinct scores per type) is tests/golden/evaluator_census.json, which
    tests/golden/gen_evaluator_census.py writes from the oracle alone.
The domain is walked in 1081 chunks (the hands that share their two lowest cards, at most 2 118 760), so no array of
the whole domain exists at any time.

Wall time, measured on 8 cores: test_every_hand_in_every_split 22 s (34 s with another job
on the machine), next to 180 s for the whole non-GPU suite before this file existed.  Threads: every core, 16 at most.
tests/sanitize_cpu.sh runs test_a_slice_under_threads only -- a REDUCED slice of the domain, the six chunks of SLICE
(2.3 M hands, the largest and the smallest chunk among them) -- under ASan/UBSan and under TSan.
"""
import math
import os

import numpy as np

from oracle import oracle as O
from tests import evaluator_domain as D
from tests import hostsim as H

THREADS = min(16, os.cpu_count() or 1)
SLICE = [(a, b) for a in (0, 30, 44) for b in (a + 1, 46)]   # first / middle / last chunks incl. the largest and the smallest


def _sweep(pairs):
    acc = D.ClassPairs()
    for a, b, cards in D.chunks(pairs):
        assert len(cards) == math.comb(51 - b, 5)
        keys, bad = H.eval7_splits(cards, THREADS)
        if bad is not None:
            per_split = {s: hex(int(H.eval7(D.resplit(cards[bad:bad + 1], s))[0])) for s in D.SPLITS}
            raise AssertionError("the key of %s depends on which two cards are the hole cards: %s" % (
                [O.card_str(c) for c in cards[bad]], per_split))
        acc.add(O.score_batch(cards, THREADS), keys, cards)
    return acc


def test_a_slice_under_threads():
    """six chunks; the threaded entries agree with the one-hand-per-call ones they stand in for"""
    acc = _sweep(SLICE)
    assert acc.n_hands() == sum(math.comb(51 - b, 5) for _, b in SLICE)
    acc.check_strictly_increasing()
    cards = D.chunk(44, 46)                       # the smallest chunk: 44, 46 and five of 47..51
    assert len(cards) == 1
    cards = D.chunk(40, 41)
    keys, bad = H.eval7_splits(cards, 3)
    assert bad is None
    for s in D.SPLITS:
        assert np.array_equal(H.eval7(D.resplit(cards, s)), keys), s
    assert np.array_equal(O.score_batch(cards, 3), O.score_batch(cards, 1))
    for i in range(0, len(cards), 7):
        _, ranks, typ = O.calc_score(cards[i])
        assert O.pack_score(typ, ranks) == int(O.score_batch(cards[i:i + 1])[0])


def test_chunks_partition_the_domain():
    assert sum(math.comb(51 - b, 5) for _, b in D.leading_pairs()) == D.N_HANDS
    assert len(set(D.leading_pairs())) == len(D.leading_pairs()) == 1081
    c = D.chunk(3, 40)
    assert len(np.unique(c, axis=0)) == len(c) == math.comb(11, 5)
    assert (np.diff(c.astype(np.int16), axis=1) > 0).all() and c.max() == 51 and (c[:, :2] == (3, 40)).all()


def test_every_hand_in_every_split():
    acc = _sweep(None)
    assert acc.n_hands() == D.N_HANDS == 133784560      # evaluated, not assumed: summed over the oracle's types
    acc.check_strictly_increasing()
    want = D.load_census()
    assert acc.census(O.TYPES) == want
    assert want["hands"] == 133784560 and len(acc.pairs) == want["classes"]
