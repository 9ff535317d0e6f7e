"""mcq_exact_batch_ext_seats on the GPU: bit for bit against the host build of its lane code (which
tests/test_exact_ext_seats_host.py pins to a literal walk), the all-in records of a mixed batch against
mcq_exact_batch_seats, a flop (more completions than one block has waves) and a preflop record (many blocks, 64-bit sums)
against the hero-only split-pot enumeration, the Monte-Carlo per-seat rows converging to the exact shares, the refusals
and the Python surface."""
from math import comb

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import exact_seats_cases as SC
from tests import ext_ways_cases as XC
from tests import hostsim_exact_seats as H
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
LAWS = ["reference", "uniform"]


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def w22(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 22)


@pytest.mark.parametrize("law", LAWS)
def test_mixed_batch_equals_the_host_build_and_the_all_in_entry(eng, law):
    """One call: the one-opponent cases with two all-in records between them (two kinds, two launches)."""
    code = LAWS.index(law)
    all_in = [SC.records(c, random_opponent=False) for c in (SC.TURN_GHOST, SC.THREE_LEVEL)]
    one = [SC.records(c) for c in SC.SMALL]
    recs = one[:2] + all_in[:1] + one[2:] + all_in[1:]
    q, ext = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    got = w32(eng.exact_ext_seats(q, ext, law))
    got_one = np.concatenate([got[:2], got[3:-1]])
    exp = np.stack([SC.host_row(i, c, code) for i, c in enumerate(SC.SMALL)])
    assert np.array_equal(got_one, exp)
    for row, c in zip(got_one, SC.SMALL):
        SE.check_invariants(row, SC.n_players(c))
    qa, ea = np.concatenate([r[0] for r in all_in]), np.concatenate([r[1] for r in all_in])
    assert np.array_equal(np.stack([got[2], got[-1]]), w32(eng.exact_seats(qa, ea, law)))
    assert np.array_equal(w32(eng.exact_ext_seats(qa, ea, law)), w32(eng.exact_seats(qa, ea, law)))


@pytest.mark.parametrize("law", LAWS)
def test_flop_strides_over_the_completions(eng, law):
    """C(45, 2) = 990 completions: more than the 16 waves of a block."""
    row = w32(eng.exact_ext_seats(*SC.records(SC.FLOP_TOP25), law))[0]
    assert np.array_equal(row, SC.host_row("flop", SC.FLOP_TOP25, LAWS.index(law)))
    SE.check_invariants(row, 3)


@pytest.mark.parametrize("law", LAWS)
def test_preflop_against_the_hero_only_enumeration(eng, law):
    """C(46, 5) completions of 820 candidate hands (two ghost cards): many blocks, and share sums beyond 32 bits, checked
    without a host walk."""
    case = SC.PREFLOP
    r = SC.words(w32(eng.exact_ext_seats(*SC.records(case), law))[0])
    SE.check_invariants(np.array(r, np.uint64), 3)
    assert r[0] > 0 and r[1] == 0 and max(r[4], r[7], r[10]) > 2 ** 32
    if law == "uniform":
        assert r[0] == comb(46, 5) * comb(41, 2)
    rot = [SC.records(SC.rotated(case, s)) for s in range(2)]
    _, weights = eng.exact_ext_ways(np.concatenate([x[0] for x in rot]), np.concatenate([x[1] for x in rot]), law)
    for s, w in enumerate(w22(weights)):
        assert int(w[0]) == r[0] and int(w[1]) == 0
        assert r[2 + 3 * s:5 + 3 * s] == [int(w[2]), int(w[3]), SE.hero_share_from_ways(w)], s
    assert r[2 + 3 * 2] > 0 and r[3 + 3 * 2] > 0


def test_monte_carlo_converges_to_the_exact_shares(eng):
    """200 000 iterations of hero + known hand + top-25 % opponent on a flop under the reference's law.  A seat's share is
    the mean of a per-iteration quantity in [0, 1], whose variance is at most 1/4: five standard deviations are
    5 sqrt(0.25 / runs) = 0.0056 (the bound of tests/test_seats_gpu.py)."""
    runs = 200000
    q, ext = SC.records(SC.FLOP_TOP25)
    exact = npa.seat_shares(eng.exact_ext_seats(q, ext, "reference"))[0]
    q["runs"] = runs
    mc = npa.seat_shares(eng.eval_batch_ext_seats(q, ext, 77))[0]
    bound = 5.0 * np.sqrt(0.25 / runs)
    for s in range(3):
        print("seat %d: mc %.6f exact %.6f bound %.6f" % (s, mc[s], exact[s], bound))
    assert bound == pytest.approx(0.0056, abs=5e-5)
    assert (np.abs(mc[:3] - exact[:3]) <= bound).all()
    assert exact[:3].sum() == pytest.approx(1.0, abs=1e-12) and not exact[3:].any()


def test_refusals_leave_out_untouched(eng):
    ids = SE.ids
    flop = ids(["2C", "7D", "9H"]) + [255, 255]
    q4 = npa.pack_queries([ids(["AH", "KD"])], [flop], 4, 1)
    q3 = npa.pack_queries([ids(["AH", "KD"])], [flop], 3, 1)
    known = [ids(["QS", "QC"])]
    good = (q3, npa.pack_query_ext(1, known=known))
    refused = [(q4, npa.pack_query_ext(1, known=known), 0),                                         # two random opponents
               (q3, npa.pack_query_ext(1, known=known, hero_range=npa.range_bits(["AKO"])), 0),     # a hero range
               (q3, npa.pack_query_ext(1, known=[npa.range_bits(["QQ"])]), 0),                      # a ranged known hand
               XC.records(XC.UNDEALABLE, 1) + (0,),                                                 # an undealable range
               (npa.pack_queries([ids(["AC", "QD"])], [ids(["AD", "AH", "KS"]) + [255, 255]], 3, 1),     # likewise, ONE opponent:
                npa.pack_query_ext(1, known=[ids(["AS", "2C"])], opp_range=npa.range_bits(XC.UNDEALABLE["opp"])), 0),   # no ace left
               good + (2,)]                                                                         # a bad law
    for q, ext, law in refused:
        out = np.full(32, SENTINEL, np.uint64)
        rc = eng._lib.mcq_exact_batch_ext_seats(eng._ctx, q.ctypes.data, ext.ctypes.data, 1, law, out.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (out == SENTINEL).all()
        if law == 0:
            with pytest.raises(ValueError):
                H.exact(q, ext, 0)
            with pytest.raises(ValueError):
                eng.exact_ext_seats(q, ext)
    # a refusal inside a batch: nothing is written for the records before it either
    out = np.full(64, SENTINEL, np.uint64)
    q, ext = np.concatenate([good[0], q4]), np.concatenate([good[1], refused[0][1]])
    rc = eng._lib.mcq_exact_batch_ext_seats(eng._ctx, q.ctypes.data, ext.ctypes.data, 2, 0, out.ctypes.data)
    assert rc == _lib.MCQ_EINVAL and (out == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.exact_ext_seats(good[0], good[1], "production")
    row = w32(eng.exact_ext_seats(*good))[0]      # the same context goes on
    assert int(row[0]) > 0
    SE.check_invariants(row, 3)


def test_get_seat_equities_exact():
    eng = _lib.default_engine()
    hands, board, ghost, opp = SC.TURN_GHOST_TOP25
    for law in LAWS:
        got = mh.get_seat_equities_exact(hands, board, 3, ghost_cards=ghost, opponent_range=0.25, dealing=law)
        assert len(got) == 3 and all(isinstance(x, float) for x in got) and sum(got) == pytest.approx(1.0, abs=1e-12)
        rows = eng.exact_ext_seats(*SC.records(SC.TURN_GHOST_TOP25), law)
        assert got == [float(x) for x in npa.seat_shares(rows)[0, :3]]
    # a set of classes as the range, and the all-in default
    assert mh.get_seat_equities_exact(hands, board, 3, ghost_cards=ghost, opponent_range=set(opp)) == \
        mh.get_seat_equities_exact(hands, board, 3, ghost_cards=ghost, opponent_range=0.25)
    assert mh.get_seat_equities_exact(hands, board, ghost_cards=ghost) == \
        mh.get_seat_equities(hands, board, ghost_cards=ghost, exact=True)
    with pytest.raises(ValueError):
        mh.get_seat_equities_exact(hands, board, 4)
