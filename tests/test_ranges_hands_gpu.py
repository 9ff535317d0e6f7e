"""mcq_eval_batch_ranges_hands on the GPU: rows per hand and per seat bit for bit the host build of the lane code with the
block tally (tests/hostsim_ranges_hands, itself held to the recount of the dealt hands in tests/test_ranges_hands_host.py);
`out` bit for bit mcq_eval_batch_ranges; one block on several records, one record over many blocks, the flush in the middle
of a record; the law per hand heads-up against the exact weighted enumeration; the refusals; the Python surface."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hostsim_ranges_hands as HH
from tests import lawstats as LS
from tests.test_ranges_gpu import BOARD, RUNS, TABLES, record

pytestmark = pytest.mark.gpu
SEED, QID = 20261021, 2000
SENTINEL = 0xABABABABABABABAB
UNIT = 2520


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def h4(hands):
    return np.ascontiguousarray(hands).view(np.uint64).reshape(-1, 1326, 4)


def batch(specs):
    recs = [record(*s) for s in specs]
    return np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])


def check_sums(rows, hands, seat):
    """contract 3, for every record of a call"""
    for r, h in zip(w32(rows), h4(hands)):
        s = h.astype(object).sum(0)
        assert [int(x) for x in s] == [int(r[0]), int(r[2 + 3 * seat]), int(r[3 + 3 * seat]), int(r[4 + 3 * seat])]


@pytest.mark.parametrize("nb", (0, 3))
@pytest.mark.parametrize("p", (2, 10))
def test_batch_of_five_equals_the_host_build(eng, nb, p):
    q, st = batch([(nb, p, r) for r in RUNS])
    plain = w32(eng.eval_batch_ranges(q, st, TABLES, SEED, first_query_id=QID))
    for seat in (0, p - 1):
        exp_rows, exp_hands = HH.run_batch(q, np.where(st == 0xFFFFFFFF, 0, st), TABLES, SEED, QID, seat)
        rows, hands = eng.eval_batch_ranges_hands(q, st, TABLES, SEED, first_query_id=QID, seat=seat)
        assert np.array_equal(w32(rows), exp_rows), (nb, p, seat)
        assert np.array_equal(h4(hands), exp_hands), (nb, p, seat)
        assert np.array_equal(w32(rows), plain)   # contract 1: out is mcq_eval_batch_ranges's row
        check_sums(rows, hands, seat)


def test_single_records_and_a_batch_mixed_over_streets_and_seats(eng):
    mix = [(0, 10, 17), (3, 2, 2500), (4, 6, 1025), (5, 3, 1), (3, 10, 1024)]
    q, st = batch(mix)
    f, seat = QID + 50, 1
    exp_rows, exp_hands = HH.run_batch(q, np.where(st == 0xFFFFFFFF, 0, st), TABLES, SEED, f, seat, grid=3)
    rows, hands = eng.eval_batch_ranges_hands(q, st, TABLES, SEED, first_query_id=f, seat=seat)
    assert np.array_equal(w32(rows), exp_rows) and np.array_equal(h4(hands), exp_hands)
    assert np.array_equal(w32(rows), w32(eng.eval_batch_ranges(q, st, TABLES, SEED, first_query_id=f)))
    check_sums(rows, hands, seat)
    for i in range(len(mix)):   # row i of the batch is the single call at id f + i
        r1, h1 = eng.eval_batch_ranges_hands(q[i:i + 1], st[i:i + 1], TABLES, SEED, first_query_id=f + i, seat=seat)
        assert np.array_equal(w32(r1)[0], exp_rows[i]) and np.array_equal(h4(h1)[0], exp_hands[i]), mix[i]
    # the batch split in two with the matching first_query_id
    ra, ha = eng.eval_batch_ranges_hands(q[:2], st[:2], TABLES, SEED, first_query_id=f, seat=seat)
    rb, hb = eng.eval_batch_ranges_hands(q[2:], st[2:], TABLES, SEED, first_query_id=f + 2, seat=seat)
    assert np.array_equal(np.concatenate([h4(ha), h4(hb)]), exp_hands)
    assert np.array_equal(np.concatenate([w32(ra), w32(rb)]), exp_rows)


def test_one_block_walks_several_records(eng, monkeypatch):
    """MCQ_GRID_CAP=1: one block runs 2500, 1 and 16385 runs one after the other -- the flush and the clearing of the table
    at every record's end.  The rows are those of the uncapped call."""
    q, st = batch([(3, 6, 2500), (3, 6, 1), (3, 3, 16385)])
    want = eng.eval_batch_ranges_hands(q, st, TABLES, SEED, first_query_id=QID + 80, seat=2)
    monkeypatch.setenv("MCQ_GRID_CAP", "1")
    e = npa.Engine(0)
    try:
        got = e.eval_batch_ranges_hands(q, st, TABLES, SEED, first_query_id=QID + 80, seat=2)
    finally:
        e.close()
    assert np.array_equal(w32(got[0]), w32(want[0])) and np.array_equal(h4(got[1]), h4(want[1]))
    check_sums(got[0], got[1], 2)
    assert [int(x) for x in h4(got[1])[:, :, 0].sum(1)] == [2500, 1, 16385]


def test_one_record_over_many_blocks(eng):
    """Three seats, 60 000 runs, the default grid: 59 tasks on as many blocks, merged by the rows' atomics."""
    q, st = batch([(3, 3, 60000)])
    exp_rows, exp_hands = HH.run_batch(q, np.where(st == 0xFFFFFFFF, 0, st), TABLES, SEED, QID + 90, 1, grid=59, waves=4)
    rows, hands = eng.eval_batch_ranges_hands(q, st, TABLES, SEED, first_query_id=QID + 90, seat=1)
    assert np.array_equal(w32(rows), exp_rows) and np.array_equal(h4(hands), exp_hands)
    check_sums(rows, hands, 1)


def test_flush_in_the_middle_of_a_record(monkeypatch):
    """One block, two one-hot seats on a full table, 130 rounds and five runs: AH KC always beats TC TD, so the watched
    hand's share is 2520 * runs, above 2^32, in closed form -- only with the flush every 64 rounds does the table's uint32
    word hold it.  Every other row is zero; no trial is abandoned."""
    monkeypatch.setenv("MCQ_GRID_CAP", "1")
    e = npa.Engine(0)
    try:
        tabs = np.zeros((2, 1326), np.uint16)
        tabs[0, _lib.hand_index(44, 50)] = 3    # KC AH
        tabs[1, _lib.hand_index(32, 33)] = 1    # TC TD
        runs = 1024 * 16 * 130 + 5
        assert UNIT * runs > 2 ** 32
        q = _lib.pack_query_one([0, 0], BOARD, 2, runs)
        st = np.array([[0, 1] + [0] * 8], np.uint32)
        rows, hands = e.eval_batch_ranges_hands(q, st, tabs, SEED, first_query_id=3, seat=0)
    finally:
        e.close()
    r, h = w32(rows)[0], h4(hands)[0]
    k = _lib.hand_index(44, 50)
    assert [int(x) for x in h[k]] == [runs, runs, 0, UNIT * runs]
    assert not np.delete(h, k, axis=0).any()
    assert int(r[0]) == runs and int(r[1]) == runs and [int(x) for x in r[2:5]] == [runs, 0, UNIT * runs]


def test_ten_distinct_full_width_tables_read_from_hbm(eng):
    """Ten distinct tables do not fit beside the table of hands: the draws read them from HBM.  The same record on one
    shared table (staged in LDS) runs in front of it in the same batch."""
    g = np.random.default_rng(11)
    tabs = g.integers(1, 8, (10, 1326)).astype(np.uint16)
    q1, _ = record(3, 10, 1025)
    q = np.concatenate([q1, q1])
    st = np.concatenate([np.zeros((1, 10), np.uint32), np.arange(10, dtype=np.uint32)[None, :]])
    exp_rows, exp_hands = HH.run_batch(q, st, tabs, SEED, QID + 69, 9)
    rows, hands = eng.eval_batch_ranges_hands(q, st, tabs, SEED, first_query_id=QID + 69, seat=9)
    assert np.array_equal(w32(rows), exp_rows) and np.array_equal(h4(hands), exp_hands)
    assert np.array_equal(w32(rows), w32(eng.eval_batch_ranges(q, st, tabs, SEED, first_query_id=QID + 69)))
    # four tables: more than the kernel stages, fewer than mcq_eval_batch_ranges's kernel does
    q4, st4 = batch([(3, 6, 1025)])
    exp_rows, exp_hands = HH.run_batch(q4, np.where(st4 == 0xFFFFFFFF, 0, st4), TABLES, SEED, 7, 5)
    rows, hands = eng.eval_batch_ranges_hands(q4, st4, TABLES, SEED, first_query_id=7, seat=5)
    assert np.array_equal(w32(rows), exp_rows) and np.array_equal(h4(hands), exp_hands)


def _weighted_pair(g, n_hands):
    t = np.zeros(1326, np.uint16)
    on = g.choice(1326, n_hands, replace=False)
    t[on] = g.integers(100, 1000, n_hands)
    return t


@pytest.mark.parametrize("nb", [3, 4], ids=["flop", "turn"])
def test_law_per_hand_heads_up_against_the_exact_weighted_enumeration(eng, nb):
    """Hero 150 hands, the opponent 200, weights in [100, 1000), 2^20 iterations.  For every hero hand h clear of the table,
    with R_h = the exact row's runs (the weight of the opponent's hands disjoint from h times the completions):
    runs_h / n against w0[h] R_h / sum, win_h / runs_h and tie_h / runs_h against the exact row, 5.5 sigma."""
    g = np.random.default_rng(200 + nb)
    w0, w1 = _weighted_pair(g, 150), _weighted_pair(g, 200)
    n = 1 << 20
    q = _lib.pack_query_one([0, 0], BOARD[:nb], 2, n)
    ext = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES, opp_range=_lib.ALL_CLASSES)
    exact, _ = eng.exact_hero_range_weighted(q, ext, w1[None, :], w0[None, :])
    r = exact[0]
    st = np.array([[0, 1] + [0] * 8], np.uint32)
    rows, hands = eng.eval_batch_ranges_hands(q, st, np.stack([w0, w1]), SEED, first_query_id=nb, seat=0)
    h = h4(hands)[0]
    on_table = set(BOARD[:nb])
    pairs = [(a, b) for b in range(52) for a in range(b)]
    allowed = [i for i, (a, b) in enumerate(pairs) if w0[i] and a not in on_table and b not in on_table]
    den = sum(int(w0[i]) * int(r["runs"][i]) for i in allowed)
    assert den > 0 and len(allowed) >= 100
    res = []
    for i in allowed:
        pm = int(w0[i]) * int(r["runs"][i]) / den
        assert pm * n >= 1000, (i, pm * n)   # the condition: every allowed hand is expected often enough to be compared
        k, win, tie = (int(x) for x in h[i, :3])
        res.append(("P(hand %d)" % i, k / n, pm, (k / n - pm) / max((pm * (1 - pm) / n) ** 0.5, 1.0 / n)))
        for name, got, ex in (("win", win, int(r["win"][i])), ("tie", tie, int(r["tie"][i]))):
            pc = ex / int(r["runs"][i])
            res.append(("%s | hand %d" % (name, i), got / k, pc, (got / k - pc) / max((pc * (1 - pc) / k) ** 0.5, 1.0 / k)))
    LS.check("law per hand heads-up, %d table cards" % nb, res)
    rest = np.delete(h, allowed, axis=0)
    assert not rest.any()   # hands of zero weight and hands on a table card: zero rows
    assert any(w0[i] and (a in on_table or b in on_table) for i, (a, b) in enumerate(pairs))   # ... and there are some
    check_sums(rows, hands, 0)


def test_refusals_leave_both_outputs_untouched(eng):
    entry = eng._lib.mcq_eval_batch_ranges_hands
    ok_q, ok_st = record(3, 3, 64)
    out = np.full((2, 32), SENTINEL, np.uint64)
    hands = np.full((2, 1326, 4), SENTINEL, np.uint64)

    def call(q, st, tb, n, seat, o=out, h=hands):
        return entry(eng._ctx, q.ctypes.data, st.ctypes.data, tb.ctypes.data, len(tb), n, SEED, 0, seat,
                     None if o is None else o.ctypes.data, None if h is None else h.ctypes.data)

    assert call(ok_q, ok_st, TABLES, 1, 3) == _lib.MCQ_EINVAL and b"no seat 3" in eng._lib.mcq_last_error()
    assert call(ok_q, ok_st, TABLES, 1, 0, h=None) == _lib.MCQ_EINVAL and b"null buffer" in eng._lib.mcq_last_error()
    assert call(ok_q, ok_st, TABLES, 1025, 0) == _lib.MCQ_EINVAL and b"MCQ_RANGES_HANDS_MAX_BATCH" in eng._lib.mcq_last_error()
    # the record whose seats block each other is seen on the device
    tabs = np.zeros((1, 1326), np.uint16)
    tabs[0, _lib.hand_index(50, 51)] = 1   # both seats hold only AH AS
    q2, st2 = record(3, 2, 64)
    q = np.concatenate([q2, _lib.pack_query_one([0, 0], [], 2, 1)])
    st = np.zeros((2, 10), np.uint32)
    tb = np.concatenate([np.ones((1, 1326), np.uint16), tabs])
    st[1, :2] = 1
    assert call(q, st, tb, 2, 0) == _lib.MCQ_EINVAL and b"block each other" in eng._lib.mcq_last_error()
    assert (out == SENTINEL).all() and (hands == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.eval_batch_ranges_hands(q, st, tb, SEED)
    with pytest.raises(ValueError):
        eng.eval_batch_ranges_hands(ok_q, ok_st, TABLES, SEED, seat=5)
    # the good record alone still runs
    rows, hh = eng.eval_batch_ranges_hands(q[:1], st[:1], tb, SEED, seat=1)
    assert int(w32(rows)[0, 0]) == 64 and int(h4(hh)[0, :, 0].sum()) == 64


def test_get_range_hand_equities_end_to_end(eng):
    ranges = [("AH", "KH"), {"QQ": 1.0, "JJ": 0.5, ("AS", "QS"): 0.25, "T9S": 1.0}, 0.25]
    flop = ["QC", "7H", "2H"]
    mh.seed(77)
    want_seats, want_trials = mh.get_range_equities(ranges, flop, runs=200000, engine=eng)
    mh.seed(77)
    seats, trials, per_hand = mh.get_range_hand_equities(ranges, flop, runs=200000, seat=1, engine=eng)
    assert seats == want_seats and trials == want_trials
    assert sum(v[0] for v in per_hand.values()) == pytest.approx(1.0, abs=1e-12)
    assert sum(v[0] * v[1] for v in per_hand.values()) == pytest.approx(seats[1][0], abs=1e-12)
    assert sum(v[0] * v[3] for v in per_hand.values()) == pytest.approx(seats[1][2], abs=1e-12)
    assert all(0.0 <= x <= 1.0 for v in per_hand.values() for x in v)
    # queens weigh twice what jacks do; neither holds the queen of clubs, which lies on the table
    assert len(per_hand) > 8 and not any("QC" in k for k in per_hand)
    for k in per_hand:
        assert npa.card_id(k[0]) < npa.card_id(k[1])
    mh.seed(77)
    _, _, known = mh.get_range_hand_equities(ranges, flop, runs=200000, seat=0, engine=eng)
    assert list(known) == [("KH", "AH")]
    assert known[("KH", "AH")] == (1.0,) + tuple(pytest.approx(x, abs=1e-12) for x in seats[0])
