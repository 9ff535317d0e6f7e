"""Per-seat rows (mcq_result_seats) without a GPU: the lane code -- mcq_iteration_ext with McqLaneAccSeats, the all-in
enumeration's mcq_exact_ext_lone_seats -- compiled for the host (tests/hostsim_seats) and pinned four ways: every seat is
recounted from the dealt hands with the oracle's comparison; runs, passes and hero's win and tie are the oracle's own
tallies; hero's share follows from the split-pot row of tests/hostsim_ext_ways; the exact weights equal a literal walk in
fractions (tests/seats_expect.py)."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import ext_ways_cases as XC
from tests import hostsim_ext_ways as HW
from tests import hostsim_seats as H
from tests import seats_expect as SE

RUNS = 4096
_seen = {"ks": set(), "other_wins": False, "cases": 0}


@pytest.mark.parametrize("i", range(len(XC.CASES)), ids=[c["name"] for c in XC.CASES])
def test_row_is_the_recount_and_hero_is_pinned(i):
    case = XC.CASES[i]
    q, ext = XC.records(case, RUNS)
    row, hands = H.run(q, ext, XC.SEED, XC.QID, hands=True)
    assert (hands != 255).all()
    assert np.array_equal(row, SE.host_row(i, RUNS, XC.SEED, XC.QID))   # (the dealt hands are a by-product, not a different walk)
    ks = set()
    assert np.array_equal(SE.seat_words(row), SE.recount(hands, case["n"], ks)), case["name"]
    oracle = XC.oracle_tallies(O.MODE_CTR, case, RUNS)
    assert [int(x) for x in row[:4]] == [int(x) for x in oracle[:4]]   # runs, passes, hero's win and tie
    ways = HW.run(False, q, ext, XC.SEED, XC.QID)
    assert [int(x) for x in row[:4]] == [int(x) for x in ways[:4]]
    assert int(row[4]) == SE.hero_share_from_ways(ways)
    SE.check_invariants(row, case["n"])
    _seen["ks"] |= ks
    _seen["other_wins"] |= bool(SE.seat_words(row)[1:, 0].any())
    _seen["cases"] += 1


def test_cases_cover_multiway_splits_and_other_winners():
    """At least three different k >= 3 occur among the cases, and some seat other than the hero wins outright."""
    if _seen["cases"] < len(XC.CASES):   # run on its own: recount here
        for i, case in enumerate(XC.CASES):
            q, ext = XC.records(case, RUNS)
            row, hands = H.run(q, ext, XC.SEED, XC.QID, hands=True)
            SE.recount(hands, case["n"], _seen["ks"])
            _seen["other_wins"] |= bool(SE.seat_words(row)[1:, 0].any())
    assert len({k for k in _seen["ks"] if k >= 3}) >= 3, _seen["ks"]
    assert _seen["other_wins"]


def test_undealable_range_is_refused():
    q, ext = XC.records(XC.UNDEALABLE, 64)
    with pytest.raises(ValueError):
        H.run(q, ext, XC.SEED, XC.QID)


def test_nothing_restricted_sums_to_one_pot():
    """Plain queries with an empty record, 2..10 players on every street: the invariants, and the hero against the
    split-pot row."""
    g = np.random.default_rng(9)
    for n in range(2, 11):
        nb = (0, 3, 4, 5)[n % 4]
        c = g.permutation(52)[:2 + nb]
        q = npa.pack_queries([c[:2]], [list(c[2:]) + [255] * (5 - nb)], n, 333)
        ext = npa.pack_query_ext(1)
        row = H.run(q, ext, 3, 40 + n)
        SE.check_invariants(row, n)
        ways = HW.run(False, q, ext, 3, 40 + n)
        assert [int(x) for x in row[:4]] == [int(x) for x in ways[:4]] and int(row[4]) == SE.hero_share_from_ways(ways)


# ---- the all-in enumeration
@pytest.mark.parametrize("law", [0, 1], ids=["reference", "uniform"])
@pytest.mark.parametrize("ci", range(len(SE.EXACT_SMALL)))
def test_exact_weights_against_the_literal_walk(ci, law):
    case = SE.EXACT_SMALL[ci]
    q, ext = SE.exact_records(case)
    SE.assert_exact_row(H.exact(q, ext, law), case, law)


def test_exact_cases_are_what_they_claim():
    sizes = {(len(c[0]), len(c[1])) for c in SE.EXACT_SMALL}
    assert {n for n, _ in sizes} == {2, 3, 6, 10} and {b for _, b in sizes} == {3, 4, 5}
    assert any(c[2] for c in SE.EXACT_SMALL) and any(not c[2] for c in SE.EXACT_SMALL)
    ak = [c for c in SE.EXACT_SMALL if c[0] == [["AH", "KD"], ["AS", "KC"], ["AD", "KH"]] and len(c[1]) == 3]
    assert ak
    for law in (0, 1):
        # three AK hands on a flop: mostly a three-way split, sometimes a flush for one of them
        s = SE.seat_words(H.exact(*SE.exact_records(ak[0]), law))
        assert s[:3, 1].all() and len({int(x) for x in s[:3, 2]}) > 1
        # the board plays for everybody: one completion, ten hands level
        ten = [c for c in SE.EXACT_SMALL if len(c[0]) == 10 and len(c[1]) == 5][0]
        row = H.exact(*SE.exact_records(ten), law)
        assert int(row[0]) == 1 and [[int(x) for x in r] for r in SE.seat_words(row)] == [[0, 1, 252]] * 10


def test_exact_refusal_codes():
    ids = SE.ids
    flop = ids(["2C", "7D", "9H"]) + [255, 255]
    q3 = npa.pack_queries([ids(["AH", "KD"])], [flop], 3, 1)
    q2 = npa.pack_queries([ids(["AH", "KD"])], [flop], 2, 1)
    known = [ids(["QS", "QC"])]
    assert H.exact_refusal(q2, npa.pack_query_ext(1, known=known), 0) == 0
    assert H.exact_refusal(q3, npa.pack_query_ext(1, known=known), 0) == 7          # a random opponent
    assert H.exact_refusal(q2, npa.pack_query_ext(1), 0) == 7
    assert H.exact_refusal(q2, npa.pack_query_ext(1, known=known, hero_range=npa.range_bits(["AKO"])), 0) == 2
    assert H.exact_refusal(q2, npa.pack_query_ext(1, known=[npa.range_bits(["QQ"])]), 0) == 3
    assert H.exact_refusal(q2, npa.pack_query_ext(1, known=[ids(["AH", "QC"])]), 0) == 1   # hero's card named twice
    with pytest.raises(ValueError):
        H.exact(q3, npa.pack_query_ext(1, known=known), 0)
