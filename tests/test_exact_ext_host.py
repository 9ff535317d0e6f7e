"""Exact enumeration of extended queries (mcq_exact_ext.hpp) on the host: the lane code, walked as the kernel walks it
(tests/hostsim_exact_ext), equals an independent index-by-index walk of the reference (tests/exact_literal.py) -- as
rationals wherever integer weights exist, within 1e-12 otherwise -- gives mcq_exact_batch's weights for a record that
restricts nothing, and refuses what it cannot enumerate.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

from neuron_poker_amd import _lib
from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
from tests import exact_literal as X
from tests import hostsim as HS
from tests import hostsim_exact_ext as H

B = [0, 5, 10, 20, 33]          # 2C 3D 4H 7C TD
TOP25 = _opponent_range_bits(0.25)
PAIRS_AK = _lib.range_bits({"AA", "KK", "AKS", "AKO", "QQ"})   # a set range with neighbour pairs (AcAd, ...)


def _case(hero, board, n, known=(), ghost=None, rng=None):
    q = _lib.pack_query_one(hero, board, n, 1)
    e = _lib.pack_query_ext(1, ghost=ghost, known=[list(h) for h in known], opp_range=rng)
    return q, e


CASES = [  # (id, hero, board, players, known hands, ghost, range)
    ("hu-river", [48, 49], B, 2, (), None, None),
    ("hu-river-top25", [48, 49], B, 2, (), None, TOP25),
    ("hu-river-set", [40, 44], B, 2, (), None, PAIRS_AK),
    ("hu-turn-top25-ghost", [40, 44], B[:4], 2, (), [50, 51], TOP25),
    ("known1-river-top25", [48, 49], B, 3, ((1, 2),), [50, 51], TOP25),
    ("known2-river-top25", [48, 49], B, 4, ((1, 2), (3, 4)), None, TOP25),
    ("known3-turn-none", [24, 28], B[:4], 4, ((1, 2), (3, 4), (50, 51)), None, None),
    ("known2-flop-none", [40, 44], B[:3], 3, ((1, 2), (3, 4)), None, None),
    ("known1-turn-set", [24, 28], B[:4], 3, ((1, 2),), [47, 46], PAIRS_AK),
    ("highest-card-hero-AsAh", [50, 51], B, 2, (), None, TOP25),
    ("three-river-top25", [48, 49], B, 3, (), None, TOP25),
    ("three-river-set", [40, 44], B, 3, (), None, PAIRS_AK),
    ("three-known1-river-top25", [48, 49], B, 4, ((1, 2),), [50, 51], TOP25),
]


@pytest.mark.parametrize("uniform", [False, True], ids=["reference", "uniform"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_lane_code_equals_the_literal_walk(case, uniform):
    _, hero, board, n, known, ghost, rng = case
    q, e = _case(hero, board, n, known, ghost, rng)
    prob, w = H.exact_ext(q, e, uniform)
    truth = X.exact(hero, board, n, known, ghost, rng, uniform)
    assert abs(sum(truth[2:]) - truth[0] - truth[1]) == 0
    if w[0]:
        assert [Fraction(int(w[2 + i]), int(w[0])) for i in range(11)] == truth
        assert prob[0] == float(w[2]) / float(w[0]) and prob[1] == float(w[3]) / float(w[0])
        assert list(prob[2:]) == [float(x) / float(w[0]) for x in w[4:]]
    else:
        n_random = n - 1 - len(known)
        assert n_random == 2 and rng is not None and not w.any()
        assert max(abs(prob[i] - float(truth[i])) for i in range(11)) < 1e-12


@pytest.mark.parametrize("uniform", [False, True], ids=["reference", "uniform"])
@pytest.mark.parametrize("hole,board,n", [([48, 49], B, 1), ([48, 49], B, 2), ([48, 49], B, 3), ([12, 49], B[:4], 2),
                                          ([48, 49], B[:4], 3), ([12, 49], B[:3], 1), ([7, 30], B[:3], 2)])
def test_unrestricted_record_equals_the_plain_enumeration(hole, board, n, uniform):
    q, e = _case(hole, board, n)
    _, w = H.exact_ext(q, e, uniform)
    assert (w == HS.exact(q.view(np.uint8), uniform)).all()
    e["opp_range"] = _lib.ALL_CLASSES                 # every class, spelt out
    assert (H.exact_ext(q, e, uniform)[1] == w).all()


def test_refusals():
    q, e = _case([48, 49], B, 2)
    bad = e.copy()
    bad["hero_is_range"] = 1
    bad["hero_range"] = TOP25
    with pytest.raises(ValueError, match="hero range"):
        H.exact_ext(q, bad)
    q3, e3 = _case([48, 49], B, 3, known=((1, 2),))
    e3["known"]["is_range"][0, 0] = 1
    e3["known"]["range"][0, 0] = TOP25
    with pytest.raises(ValueError, match="known range"):
        H.exact_ext(q3, e3)
    q4, e4 = _case([48, 49], B, 4)
    with pytest.raises(ValueError, match="too many"):
        H.exact_ext(q4, e4)
    qd, ed = _case([48, 49], B, 2, known=((48, 3),))      # a card named twice: what mcq_eval_batch_ext refuses
    with pytest.raises(ValueError, match="invalid"):
        H.exact_ext(qd, ed)
    # AA only, one ace on the table, hero holds none: the first opponent can hold two of the three aces left, the second
    # then finds no pair of aces -- a branch of positive probability the reference would never leave
    aces = _lib.range_bits({"AA"})
    qa, ea = _case([0, 4], [48, 5, 10, 20, 33], 3, rng=aces)
    with pytest.raises(ValueError, match="cannot be dealt"):
        H.exact_ext(qa, ea)
    qa1, ea1 = _case([0, 4], [48, 5, 10, 20, 33], 2, rng=aces)   # one such opponent is fine
    assert H.exact_ext(qa1, ea1)[1][0] > 0
    qn, en = _case([50, 51], [48, 49, 10, 20, 33], 2, rng=aces)   # no ace left at all
    with pytest.raises(ValueError, match="cannot be dealt"):
        H.exact_ext(qn, en)
