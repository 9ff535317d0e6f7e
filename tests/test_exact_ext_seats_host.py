"""Exact per-seat rows with one random opponent, without a GPU: the host build of the lane code
(tests/hostsim_exact_seats) against an independent literal walk in fractions (tests/exact_seats_literal.py), against the
hero-only split-pot lane code of the same and of the rotated records, the row invariants, the C ABI and the Python
surface."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import montecarlo_hip as mh
from tests import exact_seats_cases as SC
from tests import exact_seats_literal as LIT
from tests import hostsim_exact_seats as H
from tests import hostsim_ext_ways as HW
from tests import seats_expect as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = SE.UNIT
LAWS = [0, 1]   # MCQ_LAW_REFERENCE, MCQ_LAW_UNIFORM


def literal(case, law):
    hands, board, ghost, opp = case
    return LIT.exact_seats([SE.ids(h) for h in hands], SE.ids(board), len(hands) + 1, ghost=SE.ids(ghost) if ghost else None,
                           opp_range=npa.range_bits(opp) if opp is not None else None, uniform=bool(law))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("i", range(len(SC.SMALL)), ids=SC.SMALL_IDS)
def test_host_lane_code_equals_the_literal_walk(i, law):
    case = SC.SMALL[i]
    n = SC.n_players(case)
    row = SC.host_row(i, case, law)
    r = SC.words(row)
    runs = r[0]
    assert runs > 0 and r[1] == 0
    lit = literal(case, law)
    assert len(lit) == n and sum(x[2] for x in lit) == 1
    for s, (win, tie, share) in enumerate(lit):
        assert Fraction(r[2 + 3 * s], runs) == win, (s, SC.SMALL_IDS[i])
        assert Fraction(r[3 + 3 * s], runs) == tie, (s, SC.SMALL_IDS[i])
        assert Fraction(r[4 + 3 * s], UNIT * runs) == share, (s, SC.SMALL_IDS[i])
    SE.check_invariants(row, n)


@pytest.mark.parametrize("law", LAWS)
def test_the_cases_exercise_what_they_claim(law):
    hu = SC.words(SC.host_row(0, SC.HU_RIVER, law))
    assert hu[2 + 3 * 1] > 0                                   # the random seat wins outright (any pair beats ace high)
    turn = SC.words(SC.host_row(1, SC.TURN_GHOST, law))
    assert turn[2 + 3 * 1] > 0 and turn[2 + 3 * 2] > 0         # the known queens win outright, and so does the random seat
    lvl = SC.words(SC.host_row(3, SC.THREE_LEVEL, law))
    runs = lvl[0]
    # three level seats: never a win among them, and two distinct shares per tie -- 2520 / 3 against a weaker candidate,
    # 2520 / 4 when the candidate holds the fourth ace-king: the share is strictly between tie / 4 and tie / 3
    for s in range(3):
        win, tie, share = lvl[2 + 3 * s:5 + 3 * s]
        assert win == 0 and tie > 0 and (UNIT // 4) * tie < share < (UNIT // 3) * tie
    assert lvl[3 + 3 * 3] > 0 and lvl[2 + 3 * 3] > 0 and lvl[0] == runs
    ten = SC.words(SC.host_row(4, SC.TEN_WAY, law))
    assert ten[0] > 0
    for s in range(10):
        assert ten[2 + 3 * s:5 + 3 * s] == [0, ten[0], 252 * ten[0]]   # a ten-way split: every seat's share 252 runs
    opn = SC.words(SC.host_row(5, SC.ROYAL_OPEN, law))
    assert opn[2 + 3 * 9] > 0 and opn[3 + 3 * 9] > 0                     # a spade wins outright, no spade shares ten ways
    assert all(opn[2 + 3 * s:5 + 3 * s] == [0, opn[3 + 3 * 9], 252 * opn[3 + 3 * 9]] for s in range(9))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("i", range(len(SC.SMALL)), ids=SC.SMALL_IDS)
def test_seat_0_is_the_hero_only_row(i, law):
    case = SC.SMALL[i]
    r = SC.words(SC.host_row(i, case, law))
    w = HW.exact(*SC.records(case), law)
    assert r[:4] == [int(x) for x in w[:4]]
    assert r[4] == SE.hero_share_from_ways(w)


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("i", [1, 2, 3], ids=[SC.SMALL_IDS[i] for i in (1, 2, 3)])
def test_known_seat_equals_the_rotated_record(i, law):
    """The cards the random opponent is dealt from do not depend on the order of the known hands: known seat s equals the
    hero columns of the record with hand s in front."""
    case = SC.SMALL[i]
    r = SC.words(SC.host_row(i, case, law))
    for s in range(1, len(case[0])):
        rot = SC.rotated(case, s)
        w = HW.exact(*SC.records(rot), law)
        assert int(w[0]) == r[0]
        assert r[2 + 3 * s:5 + 3 * s] == [int(w[2]), int(w[3]), SE.hero_share_from_ways(w)], s
        assert SC.words(H.exact(*SC.records(rot), law))[2:5] == r[2 + 3 * s:5 + 3 * s]


@pytest.mark.parametrize("law", LAWS)
def test_no_random_opponent_is_the_all_in_row(law):
    from tests import hostsim_seats as HS
    for case in (SC.TURN_GHOST, SC.THREE_LEVEL):
        q, ext = SC.records(case, random_opponent=False)
        assert np.array_equal(H.exact(q, ext, law), HS.exact(q, ext, law))


def test_host_refusals():
    flop = SE.ids(["2C", "7D", "9H"]) + [255, 255]
    q4 = npa.pack_queries([SE.ids(["AH", "KD"])], [flop], 4, 1)
    q3 = npa.pack_queries([SE.ids(["AH", "KD"])], [flop], 3, 1)
    known = [SE.ids(["QS", "QC"])]
    with pytest.raises(ValueError, match="two random opponents"):
        H.exact(q4, npa.pack_query_ext(1, known=known), 0)
    with pytest.raises(ValueError, match="hero range"):
        H.exact(q3, npa.pack_query_ext(1, known=known, hero_range=npa.range_bits(["AKO"])), 0)
    with pytest.raises(ValueError, match="known range"):
        H.exact(q3, npa.pack_query_ext(1, known=[npa.range_bits(["QQ"])]), 0)
    assert SC.words(H.exact(q3, npa.pack_query_ext(1, known=known), 0))[0] > 0


def test_entry_declared_exported_and_bound():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        h = f.read()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", h))
    assert "mcq_exact_batch_ext_seats" in names and hasattr(L, "mcq_exact_batch_ext_seats")
    assert "TWO random opponents" in h[h.index("mcq_exact_batch_seats("):]   # the refusal is stated where the entry is declared
    assert callable(npa.Engine.exact_ext_seats)
    assert callable(npa.get_seat_equities_exact) and npa.get_seat_equities_exact is mh.get_seat_equities_exact
    assert "get_seat_equities_exact" in mh.__all__ and "get_seat_equities_exact" in npa.__all__


def test_python_refusals_without_gpu():
    two = [["AH", "KD"], ["QS", "QC"]]
    with pytest.raises(ValueError):   # two random opponents
        mh.get_seat_equities_exact(two, ["2C", "7D", "9H"], 4)
    with pytest.raises(ValueError):   # fewer players than hands
        mh.get_seat_equities_exact(two, ["2C", "7D", "9H"], 1)
    with pytest.raises(ValueError):   # a ranged known hand
        mh.get_seat_equities_exact([["AH", "KD"], {"QQ"}], ["2C", "7D", "9H"], 3)
    with pytest.raises(ValueError):   # a hero range
        mh.get_seat_equities_exact([{"AKO"}, ["QS", "QC"]], ["2C", "7D", "9H"], 3)
    with pytest.raises(ValueError):
        mh.get_seat_equities_exact(two, ["2C", "7D", "9H"], 3, dealing="production")
    with pytest.raises(ValueError):
        mh.get_seat_equities_exact([], ["2C", "7D", "9H"])
