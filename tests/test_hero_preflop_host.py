"""The preflop hero-range exact enumeration's lane code (csrc/mcq_exact_hero_pre.hpp) on the host, no GPU: unranking at 52
cards, its rows against mcq_exact_hero.hpp's on the flop, turn and river (k <= 2) and against a deliberately different slow
reference on slices of the C(|D|, 5) completions (k = 5), the host plan's bound, and every refusal."""
import math
import random

import numpy as np
import pytest

from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hero_preflop_cases as PC
from tests import hero_range_cases as HC
from tests import hostbuild
from tests import hostsim_hero_preflop as HP
from tests import hostsim_hero_range as HS

LAWS = [0, 1]   # MCQ_LAW_REFERENCE, MCQ_LAW_UNIFORM


# ---- 1. unranking
@pytest.mark.parametrize("L", [50, 52])
def test_unrank_is_the_combinatorial_number_system(L):
    n = math.comb(L, 5)
    assert HP.lib().hs_binom(L, 5) == n and n < 2 ** 32
    rng = random.Random(5200 + L)
    idx = [0, n - 1] + [rng.randrange(n) for _ in range(20000)]
    got = HP.unrank(idx, L, 5)
    assert got[0].tolist() == [0, 1, 2, 3, 4] and got[1].tolist() == list(range(L - 5, L))
    assert (np.diff(got.astype(np.int64), axis=1) > 0).all() and int(got.max()) == L - 1      # ascending, distinct, in the deck
    for i, pos in zip(idx, got.tolist()):
        assert pos == PC.unrank(i, L, 5), (L, i)
        assert PC.rank(pos) == i
    # the intermediates of mcq_exact_binom / mcq_exact_unrank at L = 52, k = 5 (the header's static_assert)
    assert max(math.comb(c, i) * c for c in range(L) for i in range(1, 6)) < 2 ** 32
    # stepping: the successor of a completion is the next index's completion (what a block does after its first one)
    some = [i for i in idx if i < n - 1] + [math.comb(c, 5) - 1 for c in range(5, L)]      # ... and every carry into the top card
    assert np.array_equal(HP.step(HP.unrank(some, L, 5), 5), HP.unrank([i + 1 for i in some], L, 5))
    for k, Lk in ((1, 48), (2, 49)):
        every = list(range(math.comb(Lk, k) - 1))
        assert np.array_equal(HP.step(HP.unrank(every, Lk, k), k), HP.unrank([i + 1 for i in every], Lk, k))
    # unused entries: k < 5 (the generic form the k <= 2 tests run)
    assert HP.unrank([7], 49, 2)[0].tolist() == PC.unrank(7, 49, 2) + [255, 255, 255]


# ---- 2. k <= 2: the existing lane code, bit for bit
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", HC.HOST_CASES + ["flop_all"])
def test_flop_turn_river_equal_the_postflop_lane_code(name, law):
    q, x = HC.records(HC.CASES[name])
    want, want_agg = HS.hero_range(q, x, law)
    rows, agg, counts = HP.hero_pre(q, x, law)
    assert np.array_equal(rows, want), (name, law)
    assert np.array_equal(agg, want_agg), (name, law)
    hands = HC.allowed_hands(HC.CASES[name])
    assert counts[0] == len(hands) and counts[2] >= max(counts[0], counts[1])
    if name == "flop_all":
        assert counts[:3] == [1176, 1176, 1176] and counts[3] == 1176      # two groups of hero hands
    if name == "turn_ghost":
        assert counts[0] < counts[1] <= counts[2] < 990                    # both ranges cut the lists
    # a cut into three parts adds up to the whole (what the launches of a call do)
    if name in ("flop_3cls", "turn_ghost"):
        n = counts[3]
        cuts = [0, n // 3, n // 3 + 1, n]
        parts = [HP.hero_pre(q, x, law, a, b)[0] for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(parts[0] + parts[1] + parts[2], want)


# ---- 3. k = 5 on completion slices against the slow reference
def _slice_check(c, law, lo, hi, rows_wanted=None):
    q, x = HC.records(c)
    deck = HC.deck(c)
    rows, agg, counts = HP.hero_pre(q, x, law, lo, hi)
    assert agg is None and counts[3] == PC.n_boards(len(deck))
    hands = HC.allowed_hands(c)
    assert counts[0] == len(hands)
    live = np.zeros(HP.ROWS, bool)
    live[[_lib.hand_index(*h) for h in hands]] = True
    assert (rows[~live] == 0).all()
    if rows_wanted is not None:
        hands = [PC.ROW_HANDS[r] for r in rows_wanted]
    ref = HP.slow_ref(deck, PC.opp_bits(c), law, PC.unrank(lo, len(deck), 5), hi - lo, hands)
    for h, want in zip(hands, ref):
        got = rows[_lib.hand_index(*h)]
        assert np.array_equal(got, want), (law, lo, h, got, want)
    assert (ref[:, 1] == 0).all()
    return rows, ref


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("n_deck", [52, 50])
def test_completion_slices_against_the_slow_reference(n_deck, law):
    c = PC.case(PC.HOST_HERO, PC.TOP10, n_deck)
    top = max(HC.deck(c))
    assert top == (51 if n_deck == 52 else 49) and any(top in h for h in HC.allowed_hands(c))
    assert len(HC.allowed_hands(c)) == (22 if n_deck == 52 else 15)
    n = PC.n_boards(n_deck)
    spans = PC.slices(n_deck)
    assert spans[0][0] == 0 and spans[2][1] == n and all(b - a == 3000 for a, b in spans)
    some = 0
    for lo, hi in spans:
        rows, ref = _slice_check(c, law, lo, hi)
        some += int(ref[:, 0].sum())
    assert some > 0
    assert PC.unrank(n - 1, n_deck, 5) == list(range(n_deck - 5, n_deck))


@pytest.mark.parametrize("law", LAWS)
def test_unrestricted_slice_and_the_group_boundary(law):
    """Nothing restricted: all 1326 hands on every list; eight hero hands against the slow reference, among them rows 0
    and 1325 and the hands at positions 1023 and 1024 of `allowed`."""
    c = PC.case(None, None, 52)
    q, x = HC.records(c)
    order = HP.allowed_rows(q, x)
    assert order == list(range(1326))
    want = PC.boundary_hands(52)
    assert {0, 1325, order[1023], order[1024]} <= set(want) and len(set(want)) == 8
    lo = PC.n_boards(52) // 3           # its highest table card is in none of the eight hands: every one of them has weight
    hi = lo + PC.SLICE
    rows, ref = _slice_check(c, law, lo, hi, rows_wanted=want)
    assert (ref[:, 0] != 0).all()
    assert HP.hero_pre(q, x, law, lo, lo + 1)[2][:3] == [1326, 1326, 1326]
    # a row is zero iff every completion of the slice holds one of the hand's cards (uniform law: no other condition)
    if law == 1:
        masks = [sum(1 << p for p in pos) for pos in HP.unrank(np.arange(lo, hi), 52, 5).tolist()]
        for r, (a, b) in enumerate(PC.ROW_HANDS):
            h = (1 << a) | (1 << b)
            assert bool(rows[r, 0]) == any(not (m & h) for m in masks), (a, b)


def test_the_two_laws_aggregates_differ_by_more_than_the_monte_carlo_bound():
    """What the GPU test of the law rests on: for hero {AA, AKs} against {KK, QQ, AKo} the whole enumeration's aggregates
    under the two laws lie more than 2 x 5.5 sigma of a 10^8-iteration run apart in some statistic, so a run within 5.5
    sigma of one is beyond 5.5 sigma of the other."""
    c = PC.case(PC.NARROW_HERO, PC.OPP_3CLS, 52)
    q, x = HC.records(c)
    ref = HP.hero_pre(q, x, 0)[1]
    uni = HP.hero_pre(q, x, 1)[1]
    n = 1e8
    z = [abs(a - b) / max((b * (1.0 - b) / n) ** 0.5, 1.0 / n) for a, b in zip(ref, uni)]
    assert max(z) > 2 * 5.5, z
    assert abs(sum(ref[2:]) - ref[0] - ref[1]) < 1e-12 and abs(sum(uni[2:]) - uni[0] - uni[1]) < 1e-12


# ---- the host plan: a thread's 32-bit sums
def test_plan_bounds_the_completions_a_block_owns():
    L = HP.lib()
    most = L.hs_pre_max_owned()
    assert most * 2 * 1081 < 2 ** 32                     # one completion adds at most 2 x C(47, 2) to tot
    assert L.hs_pre_slice(0) == 262144 <= most           # the default
    assert L.hs_pre_slice(1) == 1 and L.hs_pre_slice(324870) == 324870
    assert L.hs_pre_slice(2598960) == most and L.hs_pre_slice(2 ** 40) == most
    # threads that share one hero hand's walk: n_g hands x share threads fit the block, a wave per hand at most
    for n_g in (1, 3, 10, 15, 16, 17, 292, 302, 512, 513, 1023, 1024):
        share = L.hs_pre_share(n_g)
        assert 1 <= share <= 64 and n_g * share <= 1024 and (share == 64 or n_g * (share + 1) > 1024), n_g
    assert L.hs_pre_owned(262144, 256) == 1024 and L.hs_pre_owned(262144, 1) == 262144 and L.hs_pre_owned(10, 3) == 4


# ---- 4. refusals
def _refused(q, x, law=0, **kw):
    with pytest.raises(ValueError) as e:
        HP.hero_pre(q, x, law, **kw)     # (checks that the outputs were left untouched)
    return str(e.value)


def test_refusals():
    c = PC.case(PC.NARROW_HERO, PC.OPP_3CLS, 50)
    q, x = HC.records(c)
    HP.hero_pre(q, x, 0, 0, 10)
    qh, xh = HC.records(c, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    assert _refused(qh, xh) == "hero is not a range"
    assert _refused(*HC.records(c, n_players=3)) == "not heads-up"
    assert _refused(*HC.records(c, n_players=1)) == "not heads-up"
    assert _refused(q, x, law=2) == "bad law"
    assert _refused(q, x, lo=5, hi=5) == "empty completion range"
    x2 = x.copy()
    x2["n_known"] = 1
    x2["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    q3 = q.copy()
    q3["n_players"] = 3
    assert _refused(q3, x2) == "known hands"
    xg = x.copy()
    xg["ghost"][0] = [HC.C("2C"), HC.C("2C")]
    assert _refused(q, xg) == "invalid"
    for field in ("hero_range", "opp_range"):
        xe = x.copy()
        xe[field] = 0
        assert _refused(q, xe) == "invalid"
    # no allowed hero hand in the deck (the generic form takes table cards): 77 with three sevens gone
    assert _refused(*HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None))) == "no allowed hero hand"
    for law in LAWS:
        assert _refused(*HC.records(({"AA"}, {"AA"}, ["AD", "AC", "7H"], None)), law=law) == "range cannot be dealt"


def test_python_refusals_and_the_class_table():
    with pytest.raises(ValueError):
        mh.get_preflop_range_equity_exact({"AKS"}, ties="half")
    with pytest.raises(ValueError):
        mh.get_preflop_range_equity_exact({"AKS"}, dealing="production")
    with pytest.raises(ValueError):
        mh.get_preflop_range_equity_exact({"AKS"}, ghost_cards=["AS"])
    with pytest.raises(ValueError):
        mh.get_preflop_range_equity_exact(set())
    # the 169-class table from per-hand values: weights add up, a class's equity is the weighted mean of its hands
    rng = random.Random(169)
    hands = {}
    for a, b in PC.ROW_HANDS:
        hands[(_lib_card(a), _lib_card(b))] = (rng.random(), 1 if b == 51 else 2)
    table = mh.preflop_class_table(hands)
    assert len(table) == 169
    assert sum(w for _, w in table.values()) == sum(w for _, w in hands.values())
    aces = [(e, w) for (a, b), (e, w) in hands.items() if a[0] == "A" and b[0] == "A"]
    assert len(aces) == 6 and table["AA"][1] == sum(w for _, w in aces) == 9
    assert table["AA"][0] == pytest.approx(sum(e * w for e, w in aces) / 9, abs=1e-15)
    assert table["AKS"][1] == 7 and table["AKO"][1] == 21 and table["72O"][1] == 24
    sub = mh.preflop_class_table({k: v for k, v in hands.items() if k in (("AC", "AD"), ("KC", "AC"))})
    assert set(sub) == {"AA", "AKS"}


def _lib_card(c):
    import neuron_poker_amd as npa
    return npa.card_str(c)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- slices at 52 and 50 cards and a whole flop, both laws -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own."""
    lines = hostbuild.run_sanitized("hostsim_hero_preflop/hs_main.cpp", "-O1", tmp_path)
    assert len(lines) == 6 and all(" rc 0," in ln for ln in lines), lines
    assert "lists 1326 1326 1326 of 2598960 completions" in lines[0] and "of 2118760 completions" in lines[2]
    # the program's flop is the host build's of the postflop lane code
    q = _lib.pack_query_one([0, 0], [51, 29, 10], 2, 1)
    pairs_and_suited_aces = ["%s%s" % (r, r) for r in "23456789TJQKA"] + ["A%sS" % r for r in "23456789TJQK"]
    x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES, opp_range=_lib.range_bits(pairs_and_suited_aces))
    for law in LAWS:
        _, agg = HS.hero_range(q, x, law)
        assert "win %.9f" % agg[0] in lines[4 + law], (lines[4 + law], agg[0])
