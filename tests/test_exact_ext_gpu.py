"""Exact enumeration of extended queries on the GPU (mcq_exact_batch_ext, mcq_exact_ext_kernel): bit for bit the host
walk of the same lane code, mcq_exact_batch's weights for a record that restricts nothing, the reference's own range
test, and the yardstick the production law of extended queries had been missing -- its Monte-Carlo against the exact
expectation."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from neuron_poker_amd.cards import card_id
from tests import hostsim_exact_ext as H
from tests.test_exact_ext_host import CASES, TOP25, PAIRS_AK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def _ids(cards):
    return [card_id(c) for c in cards]


def _qe(hero, board, n, known=(), ghost=None, rng=None):
    q = _lib.pack_query_one(hero, board, n, 1)
    e = _lib.pack_query_ext(1, ghost=ghost, known=[list(h) for h in known], opp_range=rng)
    return q, e


FLOP = [0, 5, 10]
FLOP_CASES = [
    ("flop-three-known1-top25", _ids(["9C", "8C"]), _ids(["7C", "6D", "2S"]), 4, ((50, 51),), None, TOP25),
    ("flop-hu-set-ghost", [40, 44], FLOP, 2, (), [50, 51], PAIRS_AK),
    ("flop-three-none", [48, 49], FLOP, 3, ((1, 2),), None, None),
    ("flop-three-set", [40, 44], FLOP, 3, (), None, PAIRS_AK),
]


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_gpu_equals_the_host_walk_bit_for_bit(eng, law):
    cases = [c[1:] for c in CASES] + [c[1:] for c in FLOP_CASES]
    qs, es = zip(*[_qe(*c) for c in cases])
    q, e = np.concatenate(qs), np.concatenate(es)
    prob, w = eng.exact_ext(q, e, law)
    prob2, w2 = eng.exact_ext(q, e, law)
    assert prob.tobytes() == prob2.tobytes() and w.tobytes() == w2.tobytes()      # two calls: identical
    for i, c in enumerate(cases):
        hp, hw = H.exact_ext(q[i:i + 1], e[i:i + 1], law == "uniform")
        assert (w[i:i + 1].view(np.uint64) == hw).all(), (i, c)
        assert prob[i:i + 1].view(np.float64).tobytes() == hp.tobytes(), (i, c)


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_unrestricted_record_equals_mcq_exact_batch(eng, law):
    hb = [(["AH", "KH"], [], 2), (["AH", "KH"], [], 1), (["9C", "8C"], ["7C", "6D", "2S"], 3),
          (["QS", "JS"], ["2C", "3D", "4H", "7C"], 3), (["QS", "JS"], ["2C", "3D", "4H", "7C", "TD"], 2),
          (["2C", "7D"], ["AS", "KD", "QH"], 2)]
    q = np.concatenate([_lib.pack_query_one(_ids(h), _ids(b), n, 1) for h, b, n in hb])
    e = _lib.pack_query_ext(len(q))
    prob, w = eng.exact_ext(q, e, law)
    assert w.tobytes() == eng.exact(q, law).tobytes()
    assert (prob["win"] == w["win"] / w["runs"]).all()


def test_hand_versus_hand_preflop():
    """AhAd vs KsKc, uniform law, every hand known: the two directions add up to one and share their ties."""
    e_aa, r_aa = mh.get_equity_exact(["AH", "AD"], [], 2, "uniform", known_hands=[["KS", "KC"]])
    e_kk, r_kk = mh.get_equity_exact(["KS", "KC"], [], 2, "uniform", known_hands=[["AH", "AD"]])
    assert r_aa["runs"] == r_kk["runs"] > 0 and r_aa["tie"] == r_kk["tie"]
    assert int(r_aa["win"]) + int(r_kk["win"]) + int(r_aa["tie"]) == int(r_aa["runs"])
    assert abs(e_aa - 0.82) <= 0.01, e_aa


def test_reference_range_test_exact_and_replay():
    """tests/test_montecarlo_python.py:215-232 of the reference: KsKc on 3D 9H AS 7S QH against two top-25 % opponents,
    expected 12.8 % (+-3 points there).  Replay-mode Monte-Carlo (bit-exact to the reference) agrees within 5 sigma."""
    hero, board = ["KS", "KC"], ["3D", "9H", "AS", "7S", "QH"]
    mc = mh.MonteCarlo()
    eq, types = mc.run_montecarlo([hero], board, 3, None, 1, 0, '', opponent_range=0.25, mode="exact")
    assert abs(eq - 0.128) <= 0.03, eq
    assert abs(sum(v for _, v in types) - eq) < 1e-12 and mc.result["runs"] == 0
    wins, runs = 0, 0
    for s in range(10):
        r = mh.MonteCarlo()
        r.run_montecarlo([hero], board, 3, None, 1_000_000, 0, '', opponent_range=0.25, mode="replay", seed=1000 + s)
        wins += int(r.result["win"]) + int(r.result["tie"])
        runs += int(r.result["runs"])
    assert runs == 10_000_000
    p = wins / runs
    sigma = (eq * (1 - eq) / runs) ** 0.5
    assert abs(p - eq) <= 5 * sigma, (p, eq, sigma)


@pytest.mark.parametrize("name,hero,board,n,known,rng", [
    ("preflop-top25", ["AH", "KH"], [], 2, (), 0.25),
    ("flop-known1", ["9C", "8C"], ["7C", "6D", "2S"], 3, (["AS", "AD"],), 1),
    ("river-two-ranged", ["KS", "KC"], ["3D", "9H", "AS", "7S", "QH"], 3, (), 0.25),
])
def test_production_ext_law_converges_to_exact(eng, name, hero, board, n, known, rng):
    """mcq_eval_batch_ext in MCQ_MODE_PHILOX at 4e8 iterations against the exact expectation of the reference's law:
    |delta| within 5 sigma.  A failure here is a finding about the production law of extended queries."""
    opp = mh._opponent_range_bits(rng)
    q = _lib.pack_query_one(_ids(hero), _ids(board), n, 1)
    e = _lib.pack_query_ext(1, known=[_ids(h) for h in known], opp_range=opp)
    prob, _ = eng.exact_ext(q, e, "reference")
    exact = float(prob[0]["win"] + prob[0]["tie"])
    qq = np.repeat(q, 100)
    qq["runs"] = 4_000_000
    r = eng.eval_batch_ext(qq, np.repeat(e, 100), seed=20261016)
    runs = int(r["runs"].sum())
    assert runs == 400_000_000
    p = (int(r["win"].sum()) + int(r["tie"].sum())) / runs
    sigma = (exact * (1 - exact) / runs) ** 0.5
    assert abs(p - exact) <= 5 * sigma, (name, p, exact, (p - exact) / sigma)


def test_refusals_raise_and_the_context_survives(eng):
    q, e = _qe([48, 49], [0, 5, 10, 20, 33], 2)
    bad = e.copy()
    bad["hero_is_range"] = 1
    bad["hero_range"] = TOP25
    with pytest.raises(ValueError, match="hero range"):
        eng.exact_ext(q, bad)
    q4, e4 = _qe([48, 49], [0, 5, 10, 20, 33], 4)
    with pytest.raises(ValueError, match="two random opponents"):
        eng.exact_ext(q4, e4)
    qk, ek = _qe([48, 49], [0, 5, 10, 20, 33], 3, known=((1, 2),))
    ek["known"]["is_range"][0, 0] = 1
    ek["known"]["range"][0, 0] = TOP25
    with pytest.raises(ValueError, match="known hand given as a range"):
        eng.exact_ext(qk, ek)
    qa, ea = _qe([0, 4], [48, 5, 10, 20, 33], 3, rng=_lib.range_bits({"AA"}))
    with pytest.raises(ValueError, match="cannot be dealt"):
        eng.exact_ext(qa, ea)
    with pytest.raises(ValueError):
        mh.MonteCarlo().run_montecarlo([{"AA", "KK"}], [], 2, None, 1, 0, '', mode="exact")
    with pytest.raises(ValueError):
        mh.get_equity_exact(["AH", "KH"], [], 5, opponent_range=0.25)
    prob, w = eng.exact_ext(q, e)                                  # the context still works
    assert w["runs"][0] > 0 and prob["win"][0] == w["win"][0] / w["runs"][0]
