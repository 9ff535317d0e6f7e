"""The reference chain of the ranges law tests (tests/ranges_law.py), and the law itself without a GPU: the expectation
built from all-in rows against the literal enumeration, exactly, as fractions; the conditions every case must satisfy;
the host build of the lane code (tests/hostsim_ranges) against that expectation, `passes` included.  Fixed seeds,
5.5 sigma (tests/lawstats.py): a failure is a finding about the law."""
from fractions import Fraction

import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hostsim_ranges as H
from tests import lawstats as LS
from tests import ranges_law as RL
from tests import seats_expect as SE

N_HOST = 200000
N_GPU = 1 << 20
_ref = {}


def reference(name, n):
    """(tuples, a, the joint law's expectation) of a case, its conditions asserted at n; computed once."""
    if name not in _ref:
        c = RL.CASES[name]
        tl, a = RL.tuples(c["supports"], c["board"])
        _ref[name] = (tl, a, RL.all_in_rows(tl, c["board"]))
    tl, a, rows = _ref[name]
    c = RL.CASES[name]
    return tl, a, RL.conditions(c["supports"], c["board"], tl, a, rows, n)


def test_tuples_and_the_two_laws_on_a_case_done_by_hand():
    """Seat 0 holds AA or KK, seat 1 one of three pairs of which one collides with seat 0's aces: five of the six
    products are disjoint, the joint law gives seat 0 its aces in 2 of 5 deals, the sequential law in 1 of 2."""
    s0 = {"ASAH": 1, "KSKH": 1}
    s1 = {"ASAD": 1, "QSQH": 1, "TSTH": 1}
    board = ["2C", "7D", "9H", "JS", "KC"]
    tl, a = RL.tuples((s0, s1), board)
    assert len(tl) == 5 and all(w == 1 for _, w in tl) and a == Fraction(5, 6)
    seq = RL.sequential_law((s0, s1), board)
    assert [hs for hs, _ in seq] == [hs for hs, _ in tl]
    aces = RL.hand("ASAH")
    assert sum(pr for hs, pr in seq if hs[0] == aces) == Fraction(1, 2)
    assert Fraction(sum(w for hs, w in tl if hs[0] == aces), sum(w for _, w in tl)) == Fraction(2, 5)
    # weights, and a hand on the table: eff drops it from the tuples and from the denominator of a
    tl, a = RL.tuples(({"ASAH": 3, "KCKH": 5}, {"ASAD": 2, "QSQH": 7}), board)
    assert tl == [((RL.hand("ASAH"), RL.hand("QSQH")), 21)] and a == Fraction(21, 3 * 9)
    rows = RL.all_in_rows(tl, board)
    assert RL.expect_from_all_in(tl, rows) == [(1, 0, 1), (0, 0, 0)]   # a pair of aces against a pair of queens
    with pytest.raises(AssertionError):   # unequal numbers of completions are not one case
        RL.expect_from_all_in(tl + tl, np.concatenate([rows, RL.all_in_rows(tl, board[:4])]))


@pytest.mark.parametrize("name", RL.HOST_CASES)
def test_expectation_from_all_in_rows_is_the_literal_enumeration(name):
    c = RL.CASES[name]
    tl, a, expect = reference(name, N_HOST)
    lit = RL.literal_rows(c["supports"], c["board"], exact=True)
    assert len(lit) == len(expect) == len(c["supports"])
    for s, (e, l) in enumerate(zip(expect, lit)):
        assert tuple(e) == tuple(l[:3]), (name, s)
        # the variance z_rows assumes for the share is an upper bound of the true one
        assert l[3] <= e[0] + (e[2] - e[0]) / 2 - e[2] * e[2], (name, s)
    law = RL.joint_law(c["supports"], c["board"])
    assert set(law) == {hs for hs, _ in tl}
    tot = sum(w for _, w in tl)
    assert all(law[hs] == pytest.approx(w / tot, rel=1e-12) for hs, w in tl)


@pytest.mark.parametrize("name", [k for k in RL.CASES if RL.CASES[k]["board"]])
def test_cases_satisfy_their_conditions_at_the_gpu_tests_n(name):
    """Every case with a table (the preflop reference is the GPU's: 1.4 million completions per tuple)."""
    tl, a, expect = reference(name, N_GPU)
    assert a >= Fraction(1, 4) and len(tl) <= 1100
    if name == "H6":
        assert a == 1 and len(tl) == 1


def test_conditions_refuse_a_case_that_tests_nothing():
    board = RL.CASES["L1"]["board"]
    for supports, what in (
            (({"ASAH": 1, "ASKH": 1}, {"ASAD": 1, "ASKC": 1, "ASQC": 1, "AS8C": 1, "2C2D": 1}), "acceptance"),             # a = 1/5
            (({"ASAH": 1}, {"2C2D": 1}), "no strict win or no tie"),                      # disjoint hands, no tie
            (({"ASAH": 1, "8C8D": 1}, {"2C2D": 1, "3C3D": 1}), "sequential"),             # nothing collides: one law
            (({"ASAH": 60000, "2H2S": 1}, {"ADKS": 1}), "expected events")):                     # a win seen thrice in 200 000
        tl, a = RL.tuples(supports, board)
        with pytest.raises(AssertionError, match=what):
            RL.conditions(supports, board, tl, a, RL.all_in_rows(tl, board), N_HOST)


@pytest.mark.parametrize("name", RL.HOST_CASES)
def test_host_build_deals_the_joint_law(name):
    c = RL.CASES[name]
    tl, a, expect = reference(name, N_HOST)
    p = len(c["supports"])
    tabs, st = RL.case_tables(c["supports"])
    if name == "L2":
        assert st == [0, 1, 0, 2]
    q = _lib.pack_query_one([0, 0], [RL.cid(x) for x in c["board"]], p, N_HOST)
    row = H.run(q, st, tabs, 20261020, 11)
    SE.check_invariants(row, p)
    LS.check("%s host, %d tuples, a = %.4f" % (name, len(tl), float(a)), RL.z_rows(row, expect, a, N_HOST))
    if a == 1:
        assert int(row[1]) == N_HOST
    else:
        assert int(row[1]) > N_HOST


@pytest.mark.parametrize("name", ["L3", "L4", "L5", "L7", "L8"])
def test_host_build_deals_the_joint_law_on_the_flop(name):
    """Six and ten seats, known hands beside ranges, the full-width table: the cases of the GPU tests at their n, with the
    all-in rows from the oracle's scorer in the place of the GPU's enumeration."""
    c = RL.CASES[name]
    tl, a, expect = reference(name, N_GPU)
    p = len(c["supports"])
    tabs, st = RL.case_tables(c["supports"])
    q = _lib.pack_query_one([0, 0], [RL.cid(x) for x in c["board"]], p, N_GPU)
    row = H.run(q, st, tabs, 20261020, 12)
    SE.check_invariants(row, p)
    LS.check("%s host, %d tuples, a = %.4f" % (name, len(tl), float(a)), RL.z_rows(row, expect, a, N_GPU))
