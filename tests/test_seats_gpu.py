"""Per-seat rows on the GPU: mcq_eval_batch_ext_seats against the host build of the lane code (whose rows
tests/test_seats_host.py pins to the oracle and to a recount of the dealt hands) and against the split-pot entry,
mcq_exact_batch_seats against the literal walk and against the split-pot enumeration of the rotated records, the
Monte-Carlo shares against the exact ones, the refusals and the Python surface."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import ext_ways_cases as XC
from tests import hostsim_seats as H
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
RUNS = 4096
N_CASES = len(XC.CASES)
SENTINEL = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def w22(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 22)


def batch(idx, runs):
    recs = [XC.records(XC.CASES[i], runs) for i in idx]
    return np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])


def assert_hero_is_the_ways_row(seats, ways):
    for s, w in zip(seats, ways):
        assert [int(x) for x in s[:4]] == [int(x) for x in w[:4]]
        assert int(s[4]) == SE.hero_share_from_ways(w)


# ---- 1. Monte-Carlo rows against the host build
def test_cases_equal_the_host_build(eng):
    idx = list(range(N_CASES))
    q, ext = batch(idx, RUNS)
    got = w32(eng.eval_batch_ext_seats(q, ext, XC.SEED, first_query_id=XC.QID))
    exp = np.stack([SE.host_row(i, RUNS, XC.SEED, XC.QID + j) for j, i in enumerate(idx)])
    assert np.array_equal(got, exp)
    assert_hero_is_the_ways_row(got, w22(eng.eval_batch_ext_ways(q, ext, XC.SEED, first_query_id=XC.QID)))
    for row, i in zip(got, idx):
        SE.check_invariants(row, XC.CASES[i]["n"])
    # the same batch as two calls
    a = w32(eng.eval_batch_ext_seats(q[:3], ext[:3], XC.SEED, first_query_id=XC.QID))
    b = w32(eng.eval_batch_ext_seats(q[3:], ext[3:], XC.SEED, first_query_id=XC.QID + 3))
    assert np.array_equal(np.concatenate([a, b]), got)


def test_mixed_batch(eng):
    """300 extended queries: 2..10 players, every street, 200..2000 runs, a third with a known hand, a third with the
    opponents on the top half of the classes."""
    g = np.random.default_rng(17)
    B = 300
    top = npa.range_bits(XC.top_classes(0.5))
    qs, es, ns = [], [], []
    for i in range(B):
        n = int(g.integers(2, 11))
        nb = int(g.choice([0, 3, 4, 5]))
        c = [int(x) for x in g.permutation(52)[:4 + nb]]
        qs.append(npa.pack_queries([c[:2]], [c[4:] + [255] * (5 - nb)], n, int(g.integers(200, 2001))))
        es.append(npa.pack_query_ext(1, known=[c[2:4]] if i % 3 == 1 else None, opp_range=top if i % 3 == 2 else None))
        ns.append(n)
    q, ext = np.concatenate(qs), np.concatenate(es)
    got = w32(eng.eval_batch_ext_seats(q, ext, 23, first_query_id=1000))
    assert_hero_is_the_ways_row(got, w22(eng.eval_batch_ext_ways(q, ext, 23, first_query_id=1000)))
    for j in range(B):
        SE.check_invariants(got[j], ns[j])
        if j % 7 == 0:
            assert np.array_equal(got[j], H.run(q[j:j + 1], ext[j:j + 1], 23, 1000 + j)), j


def test_one_query_over_many_waves(eng):
    """20 000 iterations: the query is cut over many waves, each adding its part of the row."""
    q, ext = XC.records(XC.CASES[1], 20000)
    got = w32(eng.eval_batch_ext_seats(q, ext, XC.SEED, first_query_id=XC.QID))[0]
    assert np.array_equal(got, H.run(q, ext, XC.SEED, XC.QID))
    SE.check_invariants(got, XC.CASES[1]["n"])


# ---- 2. the all-in enumeration
@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_exact_equals_the_literal_walk(eng, law):
    recs = [SE.exact_records(c) for c in SE.EXACT_SMALL]
    q, ext = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    rows = w32(eng.exact_seats(q, ext, law))
    code = 0 if law == "reference" else 1
    for row, case in zip(rows, SE.EXACT_SMALL):
        SE.assert_exact_row(row, case, code)


PREFLOP3 = ([["AH", "KD"], ["AS", "KC"], ["QS", "QC"]], [], None)
TURN10 = ([["AH", "KD"], ["AS", "KC"], ["AD", "KH"], ["2C", "2D"], ["3C", "3D"], ["4C", "4D"], ["5C", "5D"], ["6C", "6D"],
           ["7C", "7D"], ["8C", "8D"]], ["9H", "TH", "JS", "QS"], None)


@pytest.mark.parametrize("law", ["reference", "uniform"])
@pytest.mark.parametrize("case", [PREFLOP3, TURN10], ids=["preflop3", "turn10"])
def test_exact_against_the_rotated_split_pot_enumeration(eng, case, law):
    """Seat s of the per-seat row = the hero columns of mcq_exact_batch_ext_ways for the record with hand s in front: with
    no random opponent the deck, and so the completion weights, do not depend on the order of the hands."""
    hands, board, ghost = case
    row = w32(eng.exact_seats(*SE.exact_records(case), law))[0]
    SE.check_invariants(row, len(hands))
    rot = [SE.exact_records(([hands[s]] + hands[:s] + hands[s + 1:], board, ghost)) for s in range(len(hands))]
    _, weights = eng.exact_ext_ways(np.concatenate([r[0] for r in rot]), np.concatenate([r[1] for r in rot]), law)
    for s, w in enumerate(w22(weights)):
        assert int(w[0]) == int(row[0]) and int(w[1]) == 0 == int(row[1])
        assert [int(x) for x in row[2 + 3 * s:5 + 3 * s]] == [int(w[2]), int(w[3]), SE.hero_share_from_ways(w)], s


# ---- 3. convergence
def test_convergence_to_the_exact_shares(eng):
    """200 000 iterations of the preflop three-hand case under the reference's law.  A seat's share is the mean of a
    per-iteration quantity in [0, 1], whose variance is at most 1/4: five standard deviations are 5 sqrt(0.25 / runs) =
    0.0056."""
    runs = 200000
    q, ext = SE.exact_records(PREFLOP3)
    exact = npa.seat_shares(eng.exact_seats(q, ext, "reference"))[0]
    q["runs"] = runs
    mc = npa.seat_shares(eng.eval_batch_ext_seats(q, ext, 77))[0]
    bound = 5.0 * np.sqrt(0.25 / runs)
    for s in range(3):
        print("seat %d: mc %.6f exact %.6f bound %.6f" % (s, mc[s], exact[s], bound))
    assert bound == pytest.approx(0.0056, abs=5e-5)
    assert (np.abs(mc[:3] - exact[:3]) <= bound).all()
    assert mc[:3].sum() == pytest.approx(1.0, abs=1e-12) and not mc[3:].any()


# ---- 4. refusals
def raw_seats(eng, q, ext, mode, out):
    return eng._lib.mcq_eval_batch_ext_seats(eng._ctx, q.ctypes.data, ext.ctypes.data, len(q), 1, 0, mode, out.ctypes.data)


@pytest.mark.parametrize("copies", [1, 9])
def test_undealable_range_raises_and_leaves_out_untouched(eng, copies):
    q, ext = XC.records(XC.UNDEALABLE, 64)
    q, ext = np.repeat(q, copies), np.repeat(ext, copies)
    with pytest.raises(ValueError):
        eng.eval_batch_ext_seats(q, ext, XC.SEED)
    out = np.full(copies * 32, SENTINEL, np.uint64)
    assert raw_seats(eng, q, ext, npa.MODE_PHILOX, out) == _lib.MCQ_EINVAL and (out == SENTINEL).all()


def test_invalid_query_and_parity_mode_are_refused(eng):
    q, ext = batch([0, 1], 256)
    out = np.full(2 * 32, SENTINEL, np.uint64)
    assert raw_seats(eng, q, ext, npa.MODE_REPLAY_MT19937, out) == _lib.MCQ_EINVAL and (out == SENTINEL).all()
    bad = q.copy()
    bad["hole"][1] = bad["hole"][1][0]   # the same card twice
    assert raw_seats(eng, bad, ext, npa.MODE_PHILOX, out) == _lib.MCQ_EINVAL and (out == SENTINEL).all()
    assert raw_seats(eng, q, ext, npa.MODE_PHILOX, out) == 0 and (out != SENTINEL).all()


def test_uniform_law_refused():
    e = npa.Engine(0)
    try:
        e.set_dealing_law("uniform")
        q, ext = batch([0], 256)
        out = np.full(32, SENTINEL, np.uint64)
        assert raw_seats(e, q, ext, npa.MODE_PHILOX, out) == _lib.MCQ_EINVAL and (out == SENTINEL).all()
        with pytest.raises(ValueError):
            e.eval_batch_ext_seats(q, ext, 1)
    finally:
        e.close()


def test_exact_refuses_what_it_cannot_enumerate(eng):
    ids = SE.ids
    flop = ids(["2C", "7D", "9H"]) + [255, 255]
    q3 = npa.pack_queries([ids(["AH", "KD"])], [flop], 3, 1)
    q2 = npa.pack_queries([ids(["AH", "KD"])], [flop], 2, 1)
    known = [ids(["QS", "QC"])]
    refused = [(q3, npa.pack_query_ext(1, known=known)),                                         # a random opponent
               (q2, npa.pack_query_ext(1)),                                                      # likewise, heads-up
               (q2, npa.pack_query_ext(1, known=known, hero_range=npa.range_bits(["AKO"]))),     # a hero range
               (q2, npa.pack_query_ext(1, known=[npa.range_bits(["QQ"])]))]                      # a ranged known hand
    for q, ext in refused:
        out = np.full(32, SENTINEL, np.uint64)
        rc = eng._lib.mcq_exact_batch_seats(eng._ctx, q.ctypes.data, ext.ctypes.data, 1, 0, out.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (out == SENTINEL).all()
        assert H.exact_refusal(q, ext, 0) != 0
        with pytest.raises(ValueError):
            eng.exact_seats(q, ext)
    assert int(eng.exact_seats(q2, npa.pack_query_ext(1, known=known))[0]["runs"]) > 0


# ---- 5. Python surface
def test_get_seat_equities():
    eng = _lib.default_engine()
    hands = [["AH", "KD"], ["QS", "QC"], set(XC.top_classes(0.2))]
    mh.seed(XC.SEED)
    mh.get_equity(["AH", "KH"], [], 2, 100)                                           # query id 0
    got = mh.get_seat_equities(hands, ["2C", "7D", "9H"], 5, 3000, ghost_cards=["AS", "AD"], opponent_range=0.5)   # id 1
    assert mh._stream.counter == 2
    assert len(got) == 5 and all(isinstance(x, float) for x in got) and sum(got) == pytest.approx(1.0, abs=1e-12)
    b = SE.ids(["2C", "7D", "9H"])
    q = npa.pack_queries([SE.ids(hands[0])], [b + [255, 255]], 5, 3000)
    ext = npa.pack_query_ext(1, ghost=SE.ids(["AS", "AD"]), known=[SE.ids(hands[1]), npa.range_bits(hands[2])],
                             opp_range=npa.range_bits(XC.top_classes(0.5)))
    rows = eng.eval_batch_ext_seats(q, ext, XC.SEED, first_query_id=1)
    assert got == [float(x) for x in npa.seat_shares(rows)[0, :5]]
    assert np.isnan(npa.seat_shares(rows, n_players=5)[0, 5:]).all()
    # exact: the all-in case
    ex = mh.get_seat_equities(hands[:2], ["2C", "7D", "9H"], exact=True, dealing="uniform")
    lit = SE.exact_seats_literal([SE.ids(h) for h in hands[:2]], b, uniform=True)
    assert len(ex) == 2 and sum(ex) == pytest.approx(1.0, abs=1e-12)
    assert ex == pytest.approx([float(x[2]) for x in lit], abs=1e-12)
    with pytest.raises(ValueError):
        mh.get_seat_equities(hands[:2], ["2C", "7D", "9H"], 3, exact=True)
    with pytest.raises(ValueError):
        mh.get_seat_equities(hands, ["2C", "7D", "9H"], exact=True)   # a ranged hand
