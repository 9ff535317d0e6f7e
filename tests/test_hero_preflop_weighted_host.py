"""The weighted preflop hero-range enumeration's lane code (csrc/mcq_exact_hero_pre.hpp, "weighted hands") on the host, no
GPU: its rows against the postflop weighted lane code on the flop, turn and river (k <= 2), against a literal walk of the
definition on slices of the C(|D|, 5) completions (k = 5), against the unweighted lane code when every weight is 1,
linearity in the opponent's weights, the group boundary with a holed hero table, the 64-bit sums, and every refusal."""
from fractions import Fraction

import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hero_preflop_cases as PC
from tests import hero_range_cases as HC
from tests import hostbuild
from tests import hostsim_hero_preflop as HP
from tests import hostsim_hero_preflop_weighted as HPW
from tests import hostsim_hero_weighted as HW
from tests import weighted_preflop_cases as WP
from tests import weighted_range_cases as WC

_generic = {}


def generic(name):
    """The generic lane code's (rows, agg, counts) of a postflop weighted case, computed once and left unchanged."""
    if name not in _generic:
        q, x, ow, hw = WC.records(name)
        r, a, n = HPW.hero_pre_w(q, x, ow, hw)
        r.setflags(write=False)
        _generic[name] = (r, a, n)
    return _generic[name]


# ---- 1. k <= 2: the postflop weighted lane code, bit for bit
@pytest.mark.parametrize("name", sorted(WC.WCASES))
def test_flop_turn_river_equal_the_postflop_weighted_lane_code(name):
    q, x, ow, hw = WC.records(name)
    want, want_agg = HW.hero_weighted(q, x, ow, hw)
    rows, agg, counts = generic(name)
    assert np.array_equal(rows, want), name
    assert np.array_equal(agg, want_agg), name
    base, ow1, hw1 = WC.WCASES[name]
    eff_o, eff_h = WC.effective(HC.CASES[base], ow1, hw1)
    assert counts[0] == int((eff_h != 0).sum()) == int((rows[:, 0] != 0).sum())
    assert counts[1] == int((eff_o != 0).sum()) and max(counts[0], counts[1]) <= counts[2] <= counts[0] + counts[1]
    if name == "flop_all_max":
        assert counts[:3] == [1176, 1176, 1176] and int(rows[:, 0].max()) == 1081 * 990 * WC.WMAX > 2 ** 32
    # a cut of the completions into three parts adds up to the whole (what the launches of a call do)
    if name in ("flop_3cls_hero", "turn_ghost_class"):
        n = counts[3]
        cuts = [0, n // 3, n // 3 + 1, n]
        parts = [HPW.hero_pre_w(q, x, ow, hw, a, b)[0] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(parts[0] + parts[1] + parts[2], want)


@pytest.mark.parametrize("name", ["river_hand_level", "turn_ghost_class", "flop_3cls_hero"])
def test_flop_turn_river_are_the_literal_walk(name):
    base, ow, hw = WC.WCASES[name]
    rows, agg, _ = generic(name)
    sums, lit_agg = WC.literal(HC.CASES[base], ow, hw)
    live = np.zeros(HPW.ROWS, bool)
    for h, want in sums.items():
        idx = _lib.hand_index(*h)
        live[idx] = True
        assert WC.row_ints(rows[idx]) == want, (name, h)
    assert (rows[~live] == 0).all()
    for got, want in zip(agg, lit_agg):
        assert abs(Fraction(float(got)) - want) <= Fraction(1, 10 ** 12), (name, float(got), float(want))


# ---- 2. k = 5 on completion slices against the literal walk
@pytest.mark.parametrize("n_deck", [52, 50])
def test_completion_slices_against_the_literal_walk(n_deck):
    name = "host_%d" % n_deck
    c, ow, hw = WP.WPCASES[name]
    q, x, _, _ = WP.records(name)
    hands = WP.allowed_hands(name)
    in_class = HC.allowed_hands(c)
    assert len(in_class) == (22 if n_deck == 52 else 15) and 0 < len(hands) < len(in_class)
    spans = PC.slices(n_deck)
    assert spans[0][0] == 0 and spans[2][1] == PC.n_boards(n_deck) and all(b - a == 3000 for a, b in spans)
    live = np.zeros(HPW.ROWS, bool)
    live[[_lib.hand_index(*h) for h in hands]] = True
    some = 0
    for lo, hi in spans:
        rows, agg, counts = HPW.hero_pre_w(q, x, ow, hw, lo, hi)
        assert agg is None and counts[3] == PC.n_boards(n_deck)
        lit = WP.literal_slice(c, ow, hw, lo, hi)
        assert list(lit) == hands
        for h, want in lit.items():
            got = WP.row_ints(rows[_lib.hand_index(*h)])
            assert got == want, (n_deck, lo, h, got, want)
            some += want[0]
        assert (rows[~live] == 0).all()
        # the lists are made from the tables: zeros inside allowed classes leave them
        in_opp_class = int(WC.effective(c, WC.ones(), None)[0].sum())             # the hands of the opponent's class set
        assert counts[0] == len(hands) < len(in_class)
        assert 0 < counts[1] == int((WC.effective(c, ow, hw)[0] != 0).sum()) < in_opp_class
        assert max(counts[0], counts[1]) <= counts[2] <= counts[0] + counts[1]
    assert some > 0


# ---- 3. all weights 1: the unweighted lane code under the uniform law
@pytest.mark.parametrize("n_deck", [52, 50])
def test_all_weights_one_is_the_unweighted_lane_code_bit_for_bit(n_deck):
    c = PC.case(PC.HOST_HERO, PC.TOP10, n_deck)
    q, x = HC.records(c)
    for lo, hi in PC.slices(n_deck):
        want, _, want_counts = HP.hero_pre(q, x, 1, lo, hi)
        rows, _, counts = HPW.hero_pre_w(q, x, WC.ones(), None, lo, hi)
        assert np.array_equal(rows, want) and counts[0] == want_counts[0] and counts[3] == want_counts[3], (n_deck, lo)
        # (the unweighted `live` also holds the hands that only the reference's law can deal: under the uniform law they weigh 0)
        assert counts[1] == int(WC.effective(c, WC.ones(), None)[0].sum()) <= want_counts[1]
        rows1, _, _ = HPW.hero_pre_w(q, x, WC.ones(), WC.ones(), lo, hi)        # an explicit hero table of ones: the same
        assert np.array_equal(rows1, want), (n_deck, lo)
    assert want[:, 0].any()


def test_all_weights_one_whole_flop_aggregate():
    q, x = HC.records(HC.CASES["flop_3cls"])
    want, want_agg, _ = HP.hero_pre(q, x, 1)
    rows, agg, _ = HPW.hero_pre_w(q, x, WC.ones(), None)
    assert np.array_equal(rows, want) and np.array_equal(agg, want_agg)


# ---- 4. linearity
def test_rows_are_linear_in_the_opponent_weights():
    c, _, hw = WP.WPCASES["host_52"]
    q, x, _, _ = WP.records("host_52")
    w1, w2 = (WC.hand_level(51) >> 3).astype(np.uint16), WC.class_aligned(52)
    a, b = 2, 3
    assert (w1 == 0).any() and (w2 == 0).any() and a * int(w1.max()) + b * int(w2.max()) <= WC.WMAX
    lo, hi = PC.slices(52)[1]
    r1, _, n1 = HPW.hero_pre_w(q, x, w1, hw, lo, hi)
    r2, _, n2 = HPW.hero_pre_w(q, x, w2, hw, lo, hi)
    r12, _, n12 = HPW.hero_pre_w(q, x, (a * w1 + b * w2).astype(np.uint16), hw, lo, hi)
    assert np.array_equal(r12, np.uint64(a) * r1 + np.uint64(b) * r2) and r12[:, 0].any()
    assert n12[1] > max(n1[1], n2[1])                                           # (the lists differ, the rows add up)


# ---- 5. the group boundary with holes
def test_group_boundary_with_a_holed_hero_table():
    c, ow, hw = WP.WPCASES["holed_52"]
    q, x, _, _ = WP.records("holed_52")
    order = HPW.allowed_rows(q, x, ow, hw)
    hands = WP.allowed_hands("holed_52")
    assert order == [_lib.hand_index(*h) for h in hands] and 1024 < len(order) < 1326
    assert order[1023] != 1023 and order[1024] != 1024                          # list position is not the row
    at = [0, 1, 511, 1023, 1024, 1025, len(order) - 2, len(order) - 1]
    only = [hands[i] for i in at]
    lo = PC.n_boards(52) // 3
    hi = lo + PC.SLICE
    rows, _, counts = HPW.hero_pre_w(q, x, ow, hw, lo, hi)
    eff_o = WP.effective("holed_52")[0]
    assert counts[0] == len(order) and counts[1] == int((eff_o != 0).sum()) < 12 and counts[2] == len(set(order) | set(np.flatnonzero(eff_o)))
    lit = WP.literal_slice(c, ow, hw, lo, hi, only=only)
    assert len(lit) == 8
    for h, want in lit.items():
        got = WP.row_ints(rows[_lib.hand_index(*h)])
        assert got == want and want[0] > 0, (h, got, want)
    zeroed = np.ones(HPW.ROWS, bool)
    zeroed[order] = False
    assert zeroed.sum() > 200 and (rows[zeroed] == 0).all()


# ---- 6. 64-bit sums
def test_a_long_run_of_completions_needs_the_64_bit_sums():
    """Every class against {AA, KK} at 65535: a hero hand without an ace or a king meets 12 x 65535 of weight in every
    completion that leaves all sixteen cards alone, so 6000 completions pass 2^32 in ONE host thread's sums."""
    c = PC.case(None, WP.AA_KK, 52)
    q, x = HC.records(c)
    per = 12 * WC.WMAX
    lo, hi = 0, 8 * 6000                                                          # at most eight host threads
    assert (hi - lo) // 8 * per > 2 ** 32
    plain, _, _ = HP.hero_pre(q, x, 1, lo, hi)
    rows, _, counts = HPW.hero_pre_w(q, x, WC.all_max(), None, lo, hi)
    assert counts[:3] == [1326, 12, 1326]
    assert np.array_equal(rows, plain * np.uint64(WC.WMAX))
    qq = _lib.hand_index(HC.C("QC"), HC.C("QD"))
    assert int(rows[qq, 0]) == (hi - lo) * per > 8 * 2 ** 32                      # the first completions hold low cards only


# ---- 7. refusals
def _refused(q, x, ow, hw=None, **kw):
    with pytest.raises(ValueError) as e:
        HPW.hero_pre_w(q, x, ow, hw, **kw)     # (checks that the sentinel-filled outputs were left untouched)
    return str(e.value)


def test_refusals():
    c = PC.case(PC.NARROW_HERO, PC.OPP_3CLS, 50)
    q, x = HC.records(c)
    ow = WC.ones()
    HPW.hero_pre_w(q, x, ow, None, 0, 10)
    # what the unweighted preflop host build refuses
    qh, xh = HC.records(c, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    assert _refused(qh, xh, ow) == "hero is not a range"
    assert _refused(*HC.records(c, n_players=3), ow) == "not heads-up"
    assert _refused(*HC.records(c, n_players=1), ow) == "not heads-up"
    assert _refused(q, x, ow, lo=5, hi=5) == "empty completion range"
    x2 = x.copy()
    x2["n_known"] = 1
    x2["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    q3 = q.copy()
    q3["n_players"] = 3
    assert _refused(q3, x2, ow) == "known hands"
    xg = x.copy()
    xg["ghost"][0] = [HC.C("2C"), HC.C("2C")]
    assert _refused(q, xg, ow) == "invalid"
    for field in ("hero_range", "opp_range"):
        xe = x.copy()
        xe[field] = 0
        assert _refused(q, xe, ow) == "invalid"
    assert _refused(*HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None)), ow) == "no allowed hero hand"
    assert _refused(*HC.records(({"AA"}, {"AA"}, ["AD", "AC", "7H"], None)), ow) == "range cannot be dealt"
    # no opponent table; every hero weight 0 in D -- all zero, or positive only outside the hero's classes or on hands
    # that hold a ghost card
    assert _refused(q, x, None) == "no opponent weights"
    assert _refused(q, x, ow, np.zeros(WC.ROWS, np.uint16)) == "no allowed hero hand"
    eff_h = WC.effective(c, ow, None)[1]
    outside = np.where(eff_h == 0, 9, 0).astype(np.uint16)
    assert outside.any() and _refused(q, x, ow, outside) == "no allowed hero hand"
    assert _refused(q, x, np.zeros(WC.ROWS, np.uint16)) == "range cannot be dealt"


def test_an_opponent_that_shares_a_card_is_refused_before_the_enumeration():
    """All the opponent's weight on AhAs while the hero may hold AhKh: refused by the pass over allowed x live pairs, no
    completion ranked; without the two hands that share a card with it the same table is fine."""
    q, x = HC.records(PC.case({"AKS"}, None, 52))
    ah, as_, kh, ks = HC.C("AH"), HC.C("AS"), HC.C("KH"), HC.C("KS")
    ow = np.zeros(WC.ROWS, np.uint16)
    ow[_lib.hand_index(ah, as_)] = 7
    HPW.hero_pre_w(q, x, WC.ones(), None, 0, 5)
    before = HPW.walked()
    assert before >= 5
    assert _refused(q, x, ow) == "range cannot be dealt"
    assert _refused(q, x, ow, lo=0, hi=5) == "range cannot be dealt"
    assert HPW.walked() == before
    hw = WC.ones()
    hw[[_lib.hand_index(kh, ah), _lib.hand_index(ks, as_)]] = 0
    rows, _, counts = HPW.hero_pre_w(q, x, ow, hw, 0, 5)
    assert counts[:3] == [2, 1, 3] and HPW.walked() == before + 5
    assert int((rows[:, 0] != 0).sum()) == 2 and (rows[rows[:, 0] != 0, 0] == 5 * 7).all()


# ---- 8. sanitizers
def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- slices at 52 and 50 cards and a whole ghost turn with hero weights -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own; its sums are the host build's."""
    lines = hostbuild.run_sanitized("hostsim_hero_preflop_weighted/hs_main.cpp", "-O1", tmp_path)
    assert len(lines) == 3 and all(" rc 0," in ln for ln in lines), lines
    i = np.arange(WC.ROWS, dtype=np.uint64)
    opp = np.where(i % 3 != 0, (i * 40503) & 0xFFFF, 0).astype(np.uint16)
    hero = np.where(i % 5 != 0, 1 + i % 7, 0).astype(np.uint16)
    psa = {r + r for r in "23456789TJQKA"} | {"A" + r + "S" for r in "23456789TJQK"}
    n50 = PC.n_boards(50)
    shapes = [(HC.records(PC.case(None, None, 52)), None, 0, 40),
              (HC.records((psa, psa, [], ["AH", "AS"])), hero, n50 - 500, n50),
              (HC.records((None, psa, ["AS", "9D", "4H", "QC"], ["2C", "KD"])), hero, 0, 0xFFFFFFFF)]
    for ln, (rec, hw, lo, hi) in zip(lines, shapes):
        rows, agg, counts = HPW.hero_pre_w(rec[0], rec[1], opp, hw, lo, hi)
        assert "lists %d %d %d of %d completions, %d hero hands, runs %d, win %.9f" % (
            counts[0], counts[1], counts[2], counts[3], int((rows[:, 0] != 0).sum()), int(rows[:, 0].sum()),
            0.0 if agg is None else agg[0]) in ln, ln
    # the program's turn is the postflop weighted lane code's
    rec = shapes[2][0]
    _, agg = HW.hero_weighted(rec[0], rec[1], opp, hero)
    assert "win %.9f" % agg[0] in lines[2]
