"""Writes tests/golden/evaluator_census.json: how many of the C(52,7) = 133 784 560 seven-card hands the reference's
evaluator (as restated by oracle/mcq_oracle.c, calc_score) puts into each hand type, and how many distinct scores
(type, card_ranks tuple) each type has.  From the oracle alone: nothing of the product is loaded.

    python tests/golden/gen_evaluator_census.py [threads]      (about a minute on 8 cores)

Sanity anchors.  The reference's evaluator has quirks in HOW it scores a hand, not in WHICH type it finds, so every
hand count is the textbook 7-card frequency: HighCard 23 294 460, Pair 58 627 800, TwoPair 31 433 400,
ThreeOfAKind 6 461 620, Straight 6 180 020, Flush 4 047 644, FullHouse 3 473 184, FoufOfAKind 224 848,
StraightFlush 41 584.  The numbers of distinct scores are the textbook's numbers of distinct 7-card hand values
(407, 1470, 763, 575, 10, 1277, 156 for HighCard .. FullHouse) except in two types:
  * FoufOfAKind is scored by the two highest distinct ranks of all seven cards (hand_evaluator.py:43-46), not by quad
    rank and kicker: 78 scores, not 156;
  * a StraightFlush keeps every rank of the flush suit, 5 to 8 entries with the ace counted low as well (:68-76), and
    is not reduced to the straight's top card: 298 scores, not 10.
Should a count come out otherwise, the oracle (or this note) is wrong: read hand_evaluator._calc_score before believing
either.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O                 # noqa: E402
from tests import evaluator_domain as D        # noqa: E402


def census(threads=8):
    hands = np.zeros(9, np.int64)
    scores = np.zeros(0, np.uint64)
    for _, _, cards in D.chunks():
        s = O.score_batch(cards, threads)
        hands += np.bincount(O.score_type(s), minlength=9)
        scores = np.union1d(scores, np.unique(s))
    classes = np.bincount(O.score_type(scores), minlength=9)
    assert int(hands.sum()) == D.N_HANDS
    return {"hands": int(hands.sum()), "classes": int(classes.sum()),
            "by_type": {n: {"hands": int(hands[i]), "classes": int(classes[i])} for i, n in enumerate(O.TYPES)}}


def dumps(c):
    return json.dumps(c, indent=1) + "\n"


if __name__ == "__main__":
    with open(D.CENSUS, "w") as f:
        f.write(dumps(census(int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
    print(open(D.CENSUS).read())
