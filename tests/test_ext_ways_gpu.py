"""Split-pot rows of EXTENDED queries on the GPU: mcq_eval_batch_ext_ways on every kernel path against the host build of the
lane code (whose rows tests/test_ext_ways_host.py pins to the oracle), mcq_exact_batch_ext_ways against the host lane
build, the Monte-Carlo rows against the exact weights, and the Python surface."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import ext_ways_cases as XC
from tests import hostsim_ext_ways as H
from tests.test_ext_ways_host import EXACT_SMALL, exact_records

pytestmark = pytest.mark.gpu
RUNS = 1024
N_CASES = len(XC.CASES)


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w64(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 22)


def batch(idx, runs):
    """Cases idx[0], idx[1], ... as one batch -> (queries, extension records)."""
    recs = [XC.records(XC.CASES[i], runs) for i in idx]
    return np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])


def expected(idx, runs, replay):
    """Query j of the batch has query id QID + j."""
    return np.stack([XC.hostsim_row(i, runs, replay, qid=XC.QID + j) for j, i in enumerate(idx)])


def check(eng, idx, runs, mode):
    q, ext = batch(idx, runs)
    got = w64(eng.eval_batch_ext_ways(q, ext, XC.SEED, first_query_id=XC.QID, mode=mode))
    assert np.array_equal(got, expected(idx, runs, mode == npa.MODE_REPLAY_MT19937))
    plain = np.ascontiguousarray(eng.eval_batch_ext(q, ext, XC.SEED, first_query_id=XC.QID, mode=mode))
    assert got[:, :13].tobytes() == plain.tobytes()   # words 0..12 byte-equal to the credited entry
    # invariants of every row
    assert np.array_equal(got[:, 13:22].sum(1), got[:, 3])
    for row, i in zip(got, idx):
        n = XC.CASES[i]["n"]
        assert not row[13 + n - 1:22].any()
        if n == 2:
            assert row[13] == row[3]
    return got


IDX8 = list(range(N_CASES)) + [0]
IDX14 = list(range(N_CASES)) * 2


def test_one_launch_path(eng):
    """Up to eight queries of at most 8192 iterations: one launch, fast form (cases 0, 3) and general form."""
    q, ext = batch(IDX8, RUNS)
    assert sorted({H.is_fast(q[j:j + 1], ext[j:j + 1]) for j in range(len(q))}) == [False, True]
    got = check(eng, IDX8, RUNS, npa.MODE_PHILOX)
    XC.assert_cases_vary(got)


def test_general_path_lists_staged(eng):
    """Fourteen queries: prep, lists, evaluation kernel with the block's candidate lists staged in LDS."""
    check(eng, IDX14, RUNS, npa.MODE_PHILOX)


def test_general_path_above_the_short_streams(eng):
    """More than 8192 iterations, nine queries: sixteen-iteration streams on the sliced kernel."""
    check(eng, [0, 5, 3] * 3, 9000, npa.MODE_PHILOX)


def test_general_path_staging_refused(eng):
    """Six thousand one-task queries, one of them with ten candidate lists: every block's piece of the cost axis holds
    more than 96 lists (about 23 queries x 10), so no block stages and the trials read the lists from HBM."""
    wide = dict(name="wide", hero=set(XC.top_classes(0.5)), board=[], n=10, opp=XC.top_classes(0.5),
                known=[set(XC.top_classes(0.5))] * 8)
    n, runs = 6000, 64
    recs = [XC.records(wide, runs)] + [XC.records(XC.CASES[(0, 5)[j & 1]], runs) for j in range(1, n)]
    q, ext = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    got = w64(eng.eval_batch_ext_ways(q, ext, XC.SEED, first_query_id=XC.QID))
    exp = np.stack([H.run(False, q[j:j + 1], ext[j:j + 1], XC.SEED, XC.QID + j) for j in range(n)])
    assert np.array_equal(got, exp)
    assert got[:, :13].tobytes() == np.ascontiguousarray(eng.eval_batch_ext(q, ext, XC.SEED, first_query_id=XC.QID)).tobytes()


@pytest.mark.parametrize("runs", [1, 129, 4500, 8193])
def test_replay_mode(eng, runs):
    check(eng, list(range(N_CASES)), runs, npa.MODE_REPLAY_MT19937)


@pytest.mark.parametrize("idx,cut", [(IDX8, 3), (IDX14, 5)], ids=["8", "14"])
def test_sharding_by_first_query_id(eng, idx, cut):
    q, ext = batch(idx, RUNS)
    whole = w64(eng.eval_batch_ext_ways(q, ext, XC.SEED, first_query_id=XC.QID))
    a = w64(eng.eval_batch_ext_ways(q[:cut], ext[:cut], XC.SEED, first_query_id=XC.QID))
    b = w64(eng.eval_batch_ext_ways(q[cut:], ext[cut:], XC.SEED, first_query_id=XC.QID + cut))
    assert np.array_equal(np.concatenate([a, b]), whole)


@pytest.mark.parametrize("mode", [npa.MODE_PHILOX, npa.MODE_REPLAY_MT19937], ids=["ctr", "replay"])
def test_nothing_restricted(eng, mode):
    """64 mixed plain queries with empty records: the rows of mcq_eval_batch_ways (general path, and eight of them in
    one launch)."""
    g = np.random.default_rng(5)
    B = 64
    hole = np.zeros((B, 2), np.uint8)
    board = np.full((B, 5), 255, np.uint8)
    for i in range(B):
        nb = int(g.choice([0, 3, 4, 5]))
        c = g.permutation(52)[:2 + nb]
        hole[i], board[i, :nb] = c[:2], c[2:]
    q = npa.pack_queries(hole, board, g.integers(2, 11, B).astype(np.uint8), g.integers(200, 2001, B).astype(np.uint32))
    ext = npa.pack_query_ext(B)
    for sl in (slice(0, B), slice(8, 16)):
        got = w64(eng.eval_batch_ext_ways(q[sl], ext[sl], 21, first_query_id=100, mode=mode))
        assert np.array_equal(got, w64(eng.eval_batch_ways(q[sl], 21, first_query_id=100, mode=mode)))


def test_einval_leaves_out_untouched(eng):
    q, ext = batch([0, 1], RUNS)
    q = q.copy()
    q["hole"][1] = q["hole"][1][0]   # the same card twice
    out = np.full(2 * 22, 0xABABABABABABABAB, np.uint64)
    rc = eng._lib.mcq_eval_batch_ext_ways(eng._ctx, q.ctypes.data, ext.ctypes.data, 2, 1, 0, npa.MODE_PHILOX, out.ctypes.data)
    assert rc == -1 and (out == 0xABABABABABABABAB).all()
    with pytest.raises(ValueError):
        eng.eval_batch_ext_ways(q, ext, 1)


@pytest.mark.parametrize("copies", [1, 9], ids=["one_launch", "general"])
@pytest.mark.parametrize("mode", [npa.MODE_PHILOX, npa.MODE_REPLAY_MT19937], ids=["ctr", "replay"])
def test_undealable_range_raises(eng, copies, mode):
    q, ext = XC.records(XC.UNDEALABLE, 64)
    with pytest.raises(ValueError):
        eng.eval_batch_ext_ways(np.repeat(q, copies), np.repeat(ext, copies), XC.SEED, mode=mode)


def test_uniform_law_refused():
    e = npa.Engine(0)
    try:
        e.set_dealing_law("uniform")
        q, ext = batch([0], RUNS)
        with pytest.raises(ValueError):
            e.eval_batch_ext_ways(q, ext, 1)
    finally:
        e.close()


# ---- exact entry
AKAK = (["AH", "KD"], [], 2, [["AS", "KC"]], None, None)


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_exact_equals_host_lane_build(eng, law):
    recs = [exact_records(c) for c in EXACT_SMALL]
    q, ext = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    prob, weights = eng.exact_ext_ways(q, ext, law)
    w = w64(weights)
    code = 0 if law == "reference" else 1
    assert np.array_equal(w, np.stack([H.exact(q[j:j + 1], ext[j:j + 1], code) for j in range(len(q))]))
    p13, w13 = eng.exact_ext(q, ext, law)
    assert prob["p"].tobytes() == p13.tobytes()
    assert w[:, :13].tobytes() == np.ascontiguousarray(w13).tobytes()
    assert np.array_equal(w[:, 13:22].sum(1), w[:, 3])
    assert np.array_equal(prob["tie_ways"], w[:, 13:22] / w[:, 0:1].astype(np.float64))


def test_exact_two_random_opponents_refused(eng):
    q = npa.pack_queries([[npa.card_id("AH"), npa.card_id("KD")]], [[0, 5, 10, 255, 255]], 3, 1)
    with pytest.raises(ValueError):
        eng.exact_ext_ways(q, npa.pack_query_ext(1))


def test_exact_ak_against_ak_is_half_the_pot(eng):
    """By symmetry -- under the UNIFORM law, where every completion is equally likely.  (The reference's law never deals
    the deck's highest card, here AD, to the table: that breaks the symmetry of the suits, 23154/46483 = 0.4981.)"""
    q, ext = exact_records(AKAK)
    _, weights = eng.exact_ext_ways(q, ext, "uniform")
    assert _lib.pot_share(weights, exact=True) == [Fraction(1, 2)]
    credited = (int(weights[0]["win"]) + int(weights[0]["tie"])) / int(weights[0]["runs"])
    assert credited > 0.95
    _, weights = eng.exact_ext_ways(q, ext, "reference")
    assert _lib.pot_share(weights, exact=True) == [Fraction(23154, 46483)]


def test_convergence_to_the_exact_weights(eng):
    """2^20 iterations of every case with at most one random opponent (and AhKd against AsKc).  p-hat of each
    tie_ways[k] is a binomial proportion: |p-hat - p| <= 5 sqrt(p (1 - p) / runs) + 1 / runs (five standard deviations
    and one count of rounding).  The pot share is the mean of a per-iteration value in [0, 1] with mean s, whose variance
    is at most s (1 - s): the same bound holds with s for p."""
    runs = 1 << 20
    cases = [XC.records(XC.CASES[i], runs) for i in XC.EXACT_CASES]
    ak = exact_records(AKAK)
    ak[0]["runs"] = runs
    cases.append(ak)
    q, ext = np.concatenate([r[0] for r in cases]), np.concatenate([r[1] for r in cases])
    mc = w64(eng.eval_batch_ext_ways(q, ext, 77))
    _, weights = eng.exact_ext_ways(q, ext, "reference")
    ex = w64(weights)

    def bound(p):
        return 5.0 * np.sqrt(p * (1.0 - p) / runs) + 1.0 / runs
    for m, x in zip(mc, ex):
        tot = float(x[0])
        for k in range(9):
            p = float(x[13 + k]) / tot
            print("tie_ways[%d]: mc %.6f exact %.6f bound %.6f" % (k, m[13 + k] / runs, p, bound(p)))
            assert abs(m[13 + k] / runs - p) <= bound(p)
        s = float(_lib.pot_share(x[None])[0])
        print("pot share: mc %.6f exact %.6f bound %.6f" % (_lib.pot_share(m[None])[0], s, bound(s)))
        assert abs(float(_lib.pot_share(m[None])[0]) - s) <= bound(s)


# ---- Python surface
def test_run_montecarlo_split(eng):
    case = XC.CASES[2]
    sim = mh.MonteCarlo(eng)
    eq, _ = sim.run_montecarlo([case["hero"]] + case["known"], [], case["n"], 1, maxRuns=RUNS, timeout=0, ghost_cards="",
                               seed=XC.SEED, ties="split")
    row = XC.hostsim_row(2, RUNS, False, qid=0)
    assert np.array_equal(np.array([sim.result]).view(np.uint64).reshape(22), row)
    assert eq == pytest.approx(float(_lib.pot_share(row[None])[0]), abs=1e-15)
    credited = mh.MonteCarlo(eng)
    eq_c, types_c = credited.run_montecarlo([case["hero"]] + case["known"], [], case["n"], 1, maxRuns=RUNS, timeout=0,
                                            ghost_cards="", seed=XC.SEED)
    assert eq < eq_c and dict(types_c) == dict(sim.winTypesDict)   # three AK hands: most pots hero does not lose are shared
    assert np.array_equal(np.array([credited.result]).view(np.uint64).reshape(13), row[:13])
    # mode="exact" routes to the exact ways entry
    ex = mh.MonteCarlo(eng)
    eq_x, _ = ex.run_montecarlo([["AH", "KD"], ["AS", "KC"]], [], 2, 1, maxRuns=1, timeout=0, ghost_cards="", mode="exact",
                                ties="split")
    assert eq_x == pytest.approx(23154 / 46483, abs=1e-15) and ex.result.dtype == npa.RESULT_WAYS_DTYPE


def test_get_pot_equity_keywords_and_query_ids():
    eng = _lib.default_engine()
    case = XC.CASES[3]
    mh.seed(XC.SEED)
    plain_before = mh.get_pot_equity(["AH", "KH"], [], 3, 500)                      # query id 0
    got = mh.get_pot_equity(case["hero"], case["board"], case["n"], RUNS, opponent_range=set(case["opp"]))   # id 1
    known = mh.get_pot_equity(["AH", "KD"], [], 2, RUNS, known_hands=[["AS", "KC"]])   # id 2
    assert mh._stream.counter == 3
    assert got == pytest.approx(float(_lib.pot_share(XC.hostsim_row(3, RUNS, False, qid=1)[None])[0]), abs=1e-15)
    assert 0.45 < known < 0.55
    # the default call: same entry, same query id as before the keywords existed
    q = npa.pack_queries([[npa.card_id("AH"), npa.card_id("KH")]], [[255] * 5], 3, 500)
    assert plain_before == float(_lib.pot_share(eng.eval_batch_ways(q, XC.SEED, first_query_id=0))[0])
    # ties="credited" and ties="split" consume one query id each, the same one
    for ties in ("credited", "split"):
        mh.seed(XC.SEED)
        sim = mh.MonteCarlo()
        sim.run_montecarlo([case["hero"]], case["board"], case["n"], 1, maxRuns=RUNS, timeout=0, ghost_cards="",
                           opponent_range=set(case["opp"]), ties=ties)
        assert mh._stream.counter == 1
        assert int(sim.result["win"]) == int(XC.hostsim_row(3, RUNS, False, qid=0)[2])


def test_get_equity_exact_split(eng):
    share, row = mh.get_equity_exact(["AH", "KD"], [], 2, "uniform", engine=eng, known_hands=[["AS", "KC"]], ties="split")
    assert share == 0.5 and row.dtype == npa.RESULT_WAYS_DTYPE
    credited, _ = mh.get_equity_exact(["AH", "KD"], [], 2, "uniform", engine=eng, known_hands=[["AS", "KC"]])
    assert credited > 0.95
