"""Hot boards (tests/hot_boards.py) on the host: the list proves its worth from the oracle alone, and the host build of
the kernels' lane code (tests/hostsim) -- straight-line and general iteration, both dealing laws, replay -- equals the
oracle bit for bit on the list and in every one of the 40 (players, street) instances, the headline one (6 players
before the flop: mcq_iteration<Draws, 5, 5>) included."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim as H
from tests import hot_boards as B

MODES = [O.MODE_MT, O.MODE_CTR, O.MODE_CTR_UNIFORM]
T = {n: i for i, n in enumerate(O.TYPES)}


@pytest.mark.parametrize("mode", MODES)
def test_the_list_makes_rare_shapes_common(mode):
    rows = B.expected(mode).astype(np.int64)
    assert len(rows) == len(B.SITUATIONS) * len(B.PLAYERS) and (rows[:, 0] == B.RUNS).all()
    by_type = rows[:, 4:]
    assert (by_type.sum(0) > 0).all(), dict(zip(O.TYPES, by_type.sum(0)))
    for name in ("StraightFlush", "FoufOfAKind", "FullHouse"):
        assert int((by_type[:, T[name]] > 0).sum()) >= 3, name
    assert int((rows[:, 3] > 0).sum()) * 3 >= len(rows)


def _host_rows(q, seed, qid0, **kw):
    return np.stack([H.run_ctr(q[i], seed, qid0 + i, **kw) for i in range(len(q))])


def _check(q, seed, mt_seed, qid0):
    want = O.run_batch(O.MODE_CTR, q, seed, first_qid=qid0, threads=8)
    assert np.array_equal(_host_rows(q, seed, qid0), want)
    assert np.array_equal(_host_rows(q, seed, qid0, general=True), want)
    want = O.run_batch(O.MODE_CTR_UNIFORM, q, seed, first_qid=qid0, threads=8)
    assert np.array_equal(_host_rows(q, seed, qid0, uniform=True), want)
    want = O.run_batch(O.MODE_MT, q, mt_seed, first_qid=qid0, threads=8)
    got = np.stack([H.run_replay(q[i], (mt_seed + qid0 + i) & 0xFFFFFFFF) for i in range(len(q))])
    assert np.array_equal(got, want)


def test_lane_code_on_the_list():
    _check(B.queries(), B.SEED, B.MT_SEED, B.QID)


def test_lane_code_in_all_40_instances():
    q = B.grid_queries(np.random.default_rng(40))
    cells = {(int(r[8]), int(r[7])) for r in q}
    assert cells == {(p, nb) for p in range(1, 11) for nb in (0, 3, 4, 5)}
    _check(q, B.SEED, B.MT_SEED, 1000003)
    for i in np.flatnonzero((q[:, 8] == 6) & (q[:, 7] == 0)):      # the headline instance, named: a failure says so
        want = O.run_batch(O.MODE_CTR, q[i:i + 1], B.SEED, first_qid=1000003 + int(i))
        assert np.array_equal(H.run_ctr(q[i], B.SEED, 1000003 + int(i))[None], want), "6 players before the flop"


def test_extended_lane_code_on_the_list():
    """the same situations as extended queries: a record that restricts nothing gives the plain tallies; one ranged
    opponent class set against O.run_ex"""
    import neuron_poker_amd as npa
    q = B.queries()
    plain = B.expected(O.MODE_CTR)
    free = npa.pack_query_ext(1)
    ranged = npa.pack_query_ext(1, opp_range=npa.range_bits(B.RANGE))
    for i, (hero, table, n) in enumerate(B.cases()):
        assert np.array_equal(H.run_ext(False, q[i], free, B.SEED, B.QID + i), plain[i]), (hero, table, n)
        if n > 1:
            want = O.run_ex(O.MODE_CTR, hero, table, n, B.RUNS, B.SEED, qid=B.QID + i, opp_range=B.RANGE)["tallies"]
            assert np.array_equal(H.run_ext(False, q[i], ranged, B.SEED, B.QID + i), want), (hero, table, n)
