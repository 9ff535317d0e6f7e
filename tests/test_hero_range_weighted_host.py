"""The weighted hero-range enumeration's lane code (csrc/mcq_exact_hero.hpp, "weighted hands") on the host, no GPU: its
rows and aggregate against an independent walk of the definition, against the unweighted lane code when every weight is
1, linearity in the opponent's weights, the 64-bit sums on the full flop, and the refusals."""
from fractions import Fraction

import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hero_range_cases as HC
from tests import hostbuild
from tests import hostsim_hero_range as HS
from tests import hostsim_hero_weighted as HW
from tests import weighted_range_cases as WC

_rows = {}


def rows_of(name):
    """The host build's (rows, agg) of a weighted case, computed once and left unchanged."""
    if name not in _rows:
        q, x, ow, hw = WC.records(name)
        r, a = HW.hero_weighted(q, x, ow, hw)
        r.setflags(write=False)
        _rows[name] = (r, a)
    return _rows[name]


@pytest.mark.parametrize("name", ["river_hand_level", "turn_ghost_class", "flop_3cls_hero"])
def test_rows_and_aggregate_are_the_literal_walk(name):
    base, ow, hw = WC.WCASES[name]
    case = HC.CASES[base]
    rows, agg = rows_of(name)
    sums, lit_agg = WC.literal(case, ow, hw)
    if name == "river_hand_level":
        assert len(sums) == 1081 and WC.split_classes(ow)            # every hand; suit-specific opponent weights
    if name == "turn_ghost_class":
        assert HC.AS in HC.parts(case)[2] and HC.parts(case)[3] and not WC.split_classes(ow)
    if name == "flop_3cls_hero":                                      # zeros inside the hero's three classes
        assert 0 < len(sums) < len(HC.allowed_hands(case))
    live = np.zeros(HW.ROWS, bool)
    for h, want in sums.items():
        idx = _lib.hand_index(*h)
        live[idx] = True
        got = WC.row_ints(rows[idx])
        assert got == want, (name, h, got, want)
        assert [Fraction(v, got[0]) for v in got[1:]] == [Fraction(v, want[0]) for v in want[1:]]
    assert (rows[~live] == 0).all()
    for got, want in zip(agg, lit_agg):
        assert abs(Fraction(float(got)) - want) <= Fraction(1, 10 ** 12), (name, float(got), float(want))


@pytest.mark.parametrize("name", HC.HOST_CASES)
def test_all_weights_one_is_the_unweighted_lane_code_bit_for_bit(name):
    q, x = HC.records(HC.CASES[name])
    want, want_agg = HS.hero_range(q, x, 1)
    got, got_agg = HW.hero_weighted(q, x, WC.ones(), None)
    assert np.array_equal(got, want) and np.array_equal(got_agg, want_agg), name
    got1, agg1 = HW.hero_weighted(q, x, WC.ones(), WC.ones())       # an explicit hero table of ones: the same
    assert np.array_equal(got1, want) and np.array_equal(agg1, want_agg), name


@pytest.mark.parametrize("base", ["turn_ghost", "flop_3cls"])
def test_rows_are_linear_in_the_opponent_weights(base):
    q, x = HC.records(HC.CASES[base])
    w1, w2 = WC.hand_level(21) >> 1, WC.class_aligned(22)            # (their sum stays below 65536)
    w2 = np.where(w2 == 0, 1, w2).astype(np.uint16)                  # ... and w2 alone leaves no hero hand without a row
    w1 = np.where(w1 == 0, 2, w1).astype(np.uint16)
    assert int(w1.max()) + int(w2.max()) <= WC.WMAX
    r1, _ = HW.hero_weighted(q, x, w1)
    r2, _ = HW.hero_weighted(q, x, w2)
    r12, _ = HW.hero_weighted(q, x, (w1 + w2).astype(np.uint16))
    assert np.array_equal(r12, r1 + r2) and r12[:, 0].any()


def test_full_flop_with_every_weight_65535_needs_the_64_bit_sums():
    """1081 completions x 990 opponent hands x 65535 per hero hand: 7.0e10, sixteen times what 32 bits hold."""
    q, x = HC.records(HC.CASES["flop_all"])
    plain, plain_agg = HS.hero_range(q, x, 1)
    rows, agg = rows_of("flop_all_max")
    allowed = plain[:, 0] != 0
    assert int(allowed.sum()) == 1176
    assert np.array_equal(rows, plain * np.uint64(WC.WMAX))
    assert (rows[allowed, 0] == 1081 * 990 * WC.WMAX).all() and 1081 * 990 * WC.WMAX > 2 ** 32
    assert np.allclose(agg, plain_agg, rtol=0, atol=1e-15)


def _refused(q, x, ow, hw=None):
    with pytest.raises(ValueError) as e:
        HW.hero_weighted(q, x, ow, hw)     # (checks that the sentinel-filled outputs were left untouched)
    return str(e.value)


def test_refusals():
    case = HC.CASES["turn_ghost"]
    q, x = HC.records(case)
    ow = WC.ones()
    HW.hero_weighted(q, x, ow)
    assert _refused(q, x, None) == "no opponent weights"
    qh, xh = HC.records(case, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    assert _refused(qh, xh, ow) == "hero is not a range"
    assert _refused(*HC.records(case, n_players=3), ow) == "not heads-up"
    x2 = x.copy()
    x2["n_known"] = 1
    x2["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    q3 = q.copy()
    q3["n_players"] = 3
    assert _refused(q3, x2, ow) == "known hands"
    assert _refused(_lib.pack_query_one([0, 0], [], 2, 1), x, ow) == "preflop"
    qd = q.copy()
    qd["board"][0, 1] = qd["board"][0, 0]
    assert _refused(qd, x, ow) == "invalid"
    for field in ("hero_range", "opp_range"):
        xe = x.copy()
        xe[field] = 0
        assert _refused(q, xe, ow) == "invalid"
    # no allowed hero hand: the classes leave none (77 with three sevens gone), or the weights do -- all zero, or
    # positive only outside the hero's classes or on hands that hold a table or ghost card
    assert _refused(*HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None)), ow) == "no allowed hero hand"
    assert _refused(q, x, ow, np.zeros(WC.ROWS, np.uint16)) == "no allowed hero hand"
    eff_h = WC.effective(case, ow, None)[1]
    outside = np.where(eff_h == 0, 9, 0).astype(np.uint16)
    assert outside.any() and _refused(q, x, ow, outside) == "no allowed hero hand"
    # the opponent's range cannot be dealt: by its classes, by zero weights, and against ONE hero hand only -- all the
    # weight on hands that share a card with it
    assert _refused(*HC.records(HC.UNDEALABLE), ow) == "range cannot be dealt"
    assert _refused(q, x, np.zeros(WC.ROWS, np.uint16)) == "range cannot be dealt"
    qa, xa = HC.records(HC.CASES["river_all"])
    victim = HC.allowed_hands(HC.CASES["river_all"])[500]
    sharing = np.array([1 if set(h) & set(victim) else 0 for h in WC.HANDS], np.uint16)
    assert _refused(qa, xa, sharing) == "range cannot be dealt"
    hero_without = np.array([0 if h == victim else 1 for h in WC.HANDS], np.uint16)
    rows, _ = HW.hero_weighted(qa, xa, sharing, hero_without)     # without that hand in the hero's range it is fine
    assert rows[_lib.hand_index(*victim), 0] == 0 and int((rows[:, 0] != 0).sum()) == 1080


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- a river and a ghost turn with hero weights -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own; its sums are the host build's."""
    lines = hostbuild.run_sanitized("hostsim_hero_weighted/hs_main.cpp", "-O1", tmp_path)
    assert len(lines) == 2 and all(" rc 0," in ln for ln in lines), lines
    i = np.arange(WC.ROWS, dtype=np.uint64)
    opp = np.where(i % 3 != 0, (i * 40503) & 0xFFFF, 0).astype(np.uint16)
    hero = np.where(i % 5 != 0, 1 + i % 7, 0).astype(np.uint16)
    river = HC.records((None, None, ["3C", "6D", "7H", "TS", "KC"], None))
    pairs_and_suited_aces = {r + r for r in "23456789TJQKA"} | {"A" + r + "S" for r in "23456789TJQK"}
    turn = HC.records((None, pairs_and_suited_aces, ["AS", "9D", "4H", "QC"], ["2C", "KD"]))
    for ln, (rec, hw) in zip(lines, [(river, None), (turn, hero)]):
        rows, agg = HW.hero_weighted(rec[0], rec[1], opp, hw)
        assert "%d hero hands, runs %d, win %.9f tie %.9f" % (int((rows[:, 0] != 0).sum()), int(rows[:, 0].sum()), agg[0],
                                                               agg[1]) in ln, ln
