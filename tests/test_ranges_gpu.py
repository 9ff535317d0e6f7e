"""The weighted-range-per-seat Monte-Carlo entry on the GPU (mcq_eval_batch_ranges): bit for bit the host build of its lane
code (tests/hostsim_ranges) over the streets, seat numbers and run counts at which the kernel takes another path; heads-up
against the exact weighted enumeration; the symmetry of the joint law; the contracts of the entry."""
import threading
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hostsim_ranges as H
from tests import lawstats as LS
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
SEED, QID = 20261019, 1000
SENTINEL = 0xABABABABABABABAB
BOARD = [5, 18, 31, 40, 49]   # 3D 6H 9S QC AD
# one lane, a partial stream, exactly one task, one past it, several tasks
RUNS = (1, 17, 1024, 1025, 2500)
SEATS = (2, 3, 6, 10)
STREETS = (0, 3, 4, 5)


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def _tables():
    """Three narrow tables (about 300 hands each, weights 1..9, zeros elsewhere) and a full-width one: at most six distinct
    tables per block, the form that stages them in LDS."""
    g = np.random.default_rng(7)
    t = np.zeros((4, 1326), np.uint16)
    for k in range(3):
        on = g.random(1326) < 0.23
        t[k, on] = g.integers(1, 10, int(on.sum()))
    t[3] = 1
    return t


TABLES = _tables()
_host = {}


def record(nb, p, runs):
    q = _lib.pack_query_one([0, 0], BOARD[:nb], p, runs)
    st = np.zeros((1, 10), np.uint32)
    st[0, :p] = [(s + nb) % 4 for s in range(p)]
    st[0, p:] = 0xFFFFFFFF   # not read
    return q, st


def host_row(nb, p, runs, qid, tables=None, st=None):
    key = (nb, p, runs, qid, id(tables))
    if key not in _host:
        q, s = record(nb, p, runs)
        _host[key] = H.run(q, (s if st is None else st)[0, :p], TABLES if tables is None else tables, SEED, qid)
    return _host[key]


def test_supports_accept_within_a_few_hundred_trials():
    """(CPU) ten seats on these tables: passes / runs stays far below the trial bound."""
    for nb in STREETS:
        row = host_row(nb, 10, 2500, QID + 4)
        assert int(row[1]) / int(row[0]) < 1000, (nb, row[:2])


@pytest.mark.parametrize("nb", STREETS)
@pytest.mark.parametrize("p", SEATS)
def test_batch_of_five_equals_the_host_build(eng, nb, p):
    recs = [record(nb, p, r) for r in RUNS]
    q, st = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    got = w32(eng.eval_batch_ranges(q, st, TABLES, SEED, first_query_id=QID))
    exp = np.stack([host_row(nb, p, r, QID + i) for i, r in enumerate(RUNS)])
    assert np.array_equal(got, exp), (nb, p)
    for row in got:
        SE.check_invariants(row, p)
        assert int(row[1]) >= int(row[0])


def test_single_records_and_a_batch_mixed_over_streets_and_seats(eng):
    mix = [(0, 10, 17), (3, 2, 2500), (4, 6, 1025), (5, 3, 1), (3, 10, 1024)]
    recs = [record(*m) for m in mix]
    q, st = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    exp = np.stack([host_row(nb, p, r, QID + 50 + i) for i, (nb, p, r) in enumerate(mix)])
    got = w32(eng.eval_batch_ranges(q, st, TABLES, SEED, first_query_id=QID + 50))
    assert np.array_equal(got, exp)
    for i in range(len(mix)):   # row i of the batch is the single call at id f + i
        one = w32(eng.eval_batch_ranges(q[i:i + 1], st[i:i + 1], TABLES, SEED, first_query_id=QID + 50 + i))
        assert np.array_equal(one[0], exp[i]), mix[i]
    # the batch split in two with the matching first_query_id
    a = w32(eng.eval_batch_ranges(q[:2], st[:2], TABLES, SEED, first_query_id=QID + 50))
    b = w32(eng.eval_batch_ranges(q[2:], st[2:], TABLES, SEED, first_query_id=QID + 52))
    assert np.array_equal(np.concatenate([a, b]), exp)


def test_ten_distinct_full_width_tables_read_from_hbm(eng):
    """Ten distinct tables do not fit the block's LDS beside the evaluator's: the draws read them from HBM.  The same
    record with one shared table (staged in LDS) runs next to it in the same batch."""
    g = np.random.default_rng(11)
    tabs = g.integers(1, 8, (10, 1326)).astype(np.uint16)
    q1, _ = record(3, 10, 1025)
    st = np.arange(10, dtype=np.uint32)[None, :]
    exp = H.run(q1, st[0], tabs, SEED, QID + 70)
    assert int(exp[1]) / int(exp[0]) < 1000
    got = w32(eng.eval_batch_ranges(q1, st, tabs, SEED, first_query_id=QID + 70))
    assert np.array_equal(got[0], exp)
    # both forms in one call: a first record on one table, then the ten-table record
    q = np.concatenate([q1, q1])
    st2 = np.concatenate([np.zeros((1, 10), np.uint32), st])
    exp0 = H.run(q1, st2[0], tabs, SEED, QID + 69)
    got = w32(eng.eval_batch_ranges(q, st2, tabs, SEED, first_query_id=QID + 69))
    assert np.array_equal(got[0], exp0) and np.array_equal(got[1], exp)


def test_one_long_record_over_many_tasks_per_wave(monkeypatch):
    """The per-seat wave tally (WaveTallySeats) keeps ONE 64-bit sum per lane between tasks: it has no mid-query flush and
    no threshold to cross.  What a long record does exercise is a wave adding tens of tasks of one record before its
    single flush: one block (MCQ_GRID_CAP=1), sixteen waves, forty tasks each.  p = 2, one-hot, where the host is cheap."""
    monkeypatch.setenv("MCQ_GRID_CAP", "1")
    e = npa.Engine(0)
    try:
        tabs = np.zeros((2, 1326), np.uint16)
        tabs[0, _lib.hand_index(44, 50)] = 3    # KC AH
        tabs[1, _lib.hand_index(32, 33)] = 1    # TC TD
        runs = 1024 * 16 * 40 + 5
        q = _lib.pack_query_one([0, 0], BOARD[:3], 2, runs)
        st = np.array([[0, 1] + [0] * 8], np.uint32)
        exp = H.run(q, st[0], tabs, SEED, 3)
        got = w32(e.eval_batch_ranges(q, st, tabs, SEED, first_query_id=3))
        assert np.array_equal(got[0], exp) and int(got[0, 1]) == runs
    finally:
        e.close()


def _weighted_pair(g, n_hands):
    t = np.zeros(1326, np.uint16)
    on = g.choice(1326, n_hands, replace=False)
    t[on] = g.integers(1, 1000, n_hands)
    return t


@pytest.mark.parametrize("nb", [3, 4], ids=["flop", "turn"])
def test_heads_up_against_the_exact_weighted_enumeration(eng, nb):
    """The joint expectation from Engine.exact_hero_range_weighted rows, in Python integers: runs_h is proportional to the
    weight of the opponent's hands disjoint from h, so  sum_h eff_0(h) x_h / sum_h eff_0(h) runs_h  is the joint law's."""
    g = np.random.default_rng(100 + nb)
    w0, w1 = _weighted_pair(g, 150), _weighted_pair(g, 200)
    q = _lib.pack_query_one([0, 0], BOARD[:nb], 2, 1 << 20)
    ext = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES, opp_range=_lib.ALL_CLASSES)
    rows, _ = eng.exact_hero_range_weighted(q, ext, w1[None, :], w0[None, :])
    r = rows[0]
    den = sum(int(w0[h]) * int(r["runs"][h]) for h in range(1326))
    win0 = sum(int(w0[h]) * int(r["win"][h]) for h in range(1326))
    tie = sum(int(w0[h]) * int(r["tie"][h]) for h in range(1326))
    assert den > 0
    p_win0, p_tie = win0 / den, tie / den
    p_win1 = (den - win0 - tie) / den
    st = np.array([[0, 1] + [0] * 8], np.uint32)
    got = w32(eng.eval_batch_ranges(q, st, np.stack([w0, w1]), SEED, first_query_id=nb))[0]
    n = int(got[0])
    s = SE.seat_words(got)

    def z(k, p):
        return (k / n - p) / max((p * (1 - p) / n) ** 0.5, 1.0 / n)
    LS.check("heads-up, %d table cards" % nb,
             [("seat 0 win", int(s[0, 0]) / n, p_win0, z(int(s[0, 0]), p_win0)), ("seat 0 tie", int(s[0, 1]) / n, p_tie, z(int(s[0, 1]), p_tie)),
              ("seat 1 win", int(s[1, 0]) / n, p_win1, z(int(s[1, 0]), p_win1)), ("seat 1 tie", int(s[1, 1]) / n, p_tie, z(int(s[1, 1]), p_tie))])
    assert int(s[0, 1]) == int(s[1, 1])
    SE.check_invariants(got, 2)


def test_seat_symmetry(eng):
    """Three seats, one shared table, preflop: the joint law is symmetric in the seats.  Seat a of one run against seat b of
    an INDEPENDENT run (another query id), so that the two-sample sigma is the right one."""
    q = _lib.pack_query_one([0, 0], [], 3, 1 << 19)
    st = np.zeros((3, 10), np.uint32)
    got = w32(eng.eval_batch_ranges(np.concatenate([q, q, q]), st, TABLES[:1], SEED, first_query_id=500))
    n = 1 << 19
    res = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        sa, sb = SE.seat_words(got[a])[a], SE.seat_words(got[b])[b]
        for j, name in ((0, "win"), (1, "tie")):
            p1, p2 = int(sa[j]) / n, int(sb[j]) / n
            sigma = max((p1 * (1 - p1) / n + p2 * (1 - p2) / n) ** 0.5, 1.0 / n)
            res.append(("seat %d vs seat %d %s" % (a, b, name), p1, p2, (p1 - p2) / sigma))
    LS.check("seat symmetry", res)


def test_undealable_record_returns_einval_and_leaves_out_untouched(eng):
    tabs = np.zeros((1, 1326), np.uint16)
    tabs[0, _lib.hand_index(50, 51)] = 1   # both seats hold only AH AS
    ok_q, ok_st = record(3, 2, 64)
    q = np.concatenate([ok_q, _lib.pack_query_one([0, 0], [], 2, 1)])
    st = np.zeros((2, 10), np.uint32)
    wide = np.ones((1, 1326), np.uint16)
    tb = np.concatenate([wide, tabs])
    st[1, :2] = 1
    out = np.full((2, 32), SENTINEL, np.uint64)
    rc = eng._lib.mcq_eval_batch_ranges(eng._ctx, q.ctypes.data, st.ctypes.data, tb.ctypes.data, 2, 2, SEED, 0, out.ctypes.data)
    assert rc == _lib.MCQ_EINVAL and (out == SENTINEL).all()
    assert b"block each other" in eng._lib.mcq_last_error()
    with pytest.raises(ValueError):
        eng.eval_batch_ranges(q, st, tb, SEED)
    # the good record alone still runs
    assert int(w32(eng.eval_batch_ranges(q[:1], st[:1], tb, SEED))[0, 0]) == 64


def test_second_call_on_a_busy_context_is_turned_away(eng):
    recs = [record(3, 6, 8192) for _ in range(192)]
    big = (np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs]), TABLES, SEED)
    small = record(5, 2, 64) + (TABLES, SEED)
    want_small = w32(eng.eval_batch_ranges(*small))
    want_big = w32(eng.eval_batch_ranges(*big))
    started, results, busy = threading.Event(), [], [0]

    def long_call():
        started.set()
        while not results:
            try:
                results.append(w32(eng.eval_batch_ranges(*big)))
            except npa.McqBusyError as e:      # the short call was in flight: turned away likewise, try again
                assert "context busy" in str(e)
                busy[0] += 1
    th = threading.Thread(target=long_call)
    th.start()
    started.wait()
    deadline = time.time() + 5
    while th.is_alive() and time.time() < deadline:
        try:
            assert np.array_equal(w32(eng.eval_batch_ranges(*small)), want_small)   # got in between two calls: fine
        except npa.McqBusyError as e:
            assert "context busy" in str(e)
            busy[0] += 1
    th.join()
    assert busy[0] > 0
    assert np.array_equal(results[0], want_big)
    assert np.array_equal(w32(eng.eval_batch_ranges(*small)), want_small)


def test_get_range_equities_end_to_end(eng):
    ranges = [("AH", "KH"), {"QQ": 1.0, "JJ": 0.5, ("AS", "QS"): 0.25, "T9S": 1.0}, 0.25]
    flop = ["QC", "7H", "2H"]
    mh.seed(77)
    seats, trials = mh.get_range_equities(ranges, flop, runs=200000, engine=eng)
    assert len(seats) == 3 and trials >= 1.0
    assert sum(s[2] for s in seats) == pytest.approx(1.0, abs=1e-12)
    assert all(0.0 <= w <= 1.0 and 0.0 <= t <= 1.0 and w + t <= 1.0 for w, t, _ in seats)
    tables, seat_table = mh._range_tables(ranges)
    assert len(tables) == 3
    q = _lib.pack_query_one([0, 0], [npa.card_id(c) for c in flop], 3, 200000)
    rows = eng.eval_batch_ranges(q, seat_table, tables, 77, first_query_id=0)
    r = rows[0]
    assert seats[1][0] == int(r["seat"][1]["win"]) / 200000 and trials == int(r["passes"]) / 200000
    # the nut flush draw with two overcards against a set-heavy range and a wide one: neither crushed nor crushing
    assert 0.2 < seats[0][2] < 0.6
