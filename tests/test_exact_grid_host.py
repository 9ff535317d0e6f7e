"""The exact-enumeration grid (tests/exact_grid.py) on the host: the rows the host builds of the lane code give -- what
tests/test_exact_grid_gpu.py demands of the kernels bit for bit -- are pinned here to the independent literal walks
(tests/exact_literal.py, exact_ways_literal.py, exact_seats_literal.py in fractions, oracle.exact, and a plain enumeration
scored by the oracle for the all-in preflop records), and the plans (mirrors of mcq_exact_plan / mcq_exact_ext_plan) are
shown to give a wave, lane or block several completions once MCQ_EXACT_CU caps the CU count.  No GPU needed."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import exact_grid as G
from tests import exact_literal as X
from tests import exact_seats_literal as XS
from tests import exact_ways_literal as XW
from tests import hostsim_exact_ext as H
from tests.seats_expect import check_invariants

UNIT = G.UNIT
WALKED = [r for r in G.grid() if r.literal == "walk"]
# oracle.exact sums the probabilities of up to 1.5e8 leaves in double precision: rounding stays below 1e-9 (the bound
# tests/test_gpu_parity.py holds the same comparison to)
ORACLE_TOL = 1e-9


def _ints(row):
    return [int(x) for x in np.asarray(row).reshape(-1)]


def _args(rec):
    return rec.hero, rec.board, rec.n_players, rec.known, rec.ghost, G.RANGES[rec.rng]


def test_the_grid_is_complete_and_its_records_are_what_they_say():
    recs = G.grid()
    G.assert_grid(recs)
    for r in recs:
        rid = np.zeros(64, np.uint8)
        assert H.lib().hs_exact_ext_r(C.c_void_p(r.q.ctypes.data), C.c_void_p(r.e.ctypes.data), C.c_int(0), C.c_void_p(rid.ctypes.data)) == r.L == len(r.deck()), r
        assert list(rid[:r.L]) == r.deck(), r
    for en in G.WORDS:
        assert [r for r in G.batch(en)] and {r.name for r in G.batch(en)} == {r.name for r in recs if en in r.entries}
    assert sum(1 for r in G.batch("ext") if r.kind == 2) >= 2


def test_share_of_records_held_by_a_literal_check(capsys):
    """Every (kind, row form, law) is literally walked on a river and on a turn record (the walks below run under both
    laws), every top-of-deck record is, and at most one half of the grid is left to the host build alone."""
    recs = G.grid()
    for kind, forms in ((0, ("ext", "ways", "seats", "ext_seats")), (1, ("ext", "ways", "ext_seats")), (2, ("ext",))):
        for en in forms:
            for nb in (4, 5):
                assert any(r.kind == kind and r.nb == nb and en in r.entries for r in WALKED), (kind, en, nb)
    for nb in (4, 5):   # two random opponents: the integer weights (no range) are walked too, and `exact` is held to the oracle
        assert any(r.kind == 2 and r.nb == nb and not r.restricted_range and int(G.plain_row(r, "reference")[1][0]) for r in WALKED), nb
        assert any(r.kind == 2 and r.nb == nb and "exact" in r.entries and r.literal == "oracle" for r in recs), nb
    assert all(r.literal == "walk" for r in recs if "top" in r.tags)
    left = [r for r in recs if r.literal is None]
    share = len(left) / len(recs)
    with capsys.disabled():
        print("\nexact grid: %d records, %d without a literal check (%.1f %%): %s"
              % (len(recs), len(left), 100 * share, " ".join(r.name for r in left)))
    assert share <= 0.5


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("rec", WALKED, ids=[r.name for r in WALKED])
def test_host_rows_equal_the_literal_walks(rec, law):
    uniform = law == "uniform"
    prob, w = G.plain_row(rec, law)
    w = _ints(w)
    truth = X.exact(*_args(rec), uniform)
    assert sum(truth[2:]) == truth[0] + truth[1]
    if w[0]:
        assert [Fraction(w[2 + i], w[0]) for i in range(11)] == truth
        assert list(prob) == [float(w[2 + i]) / float(w[0]) for i in range(11)]
    else:   # a range and two random opponents: no common total, the probabilities alone
        assert rec.kind == 2 and rec.rng not in ("none", "all169") and not any(w)
        assert max(abs(prob[i] - float(truth[i])) for i in range(11)) < 1e-12
    if "exact" in rec.entries:
        assert _ints(G.exact_row(rec, law)) == w
    if "ways" in rec.entries:
        row = _ints(G.ways_row(rec, law))
        win, ties = XW.exact_ways(*_args(rec), uniform)
        assert row[:13] == w and row[1] == 0
        assert Fraction(row[2], row[0]) == win and [Fraction(row[13 + j], row[0]) for j in range(9)] == ties
        assert sum(row[13:]) == row[3]
    if "ext_seats" in rec.entries:
        row = _ints(G.ext_seats_row(rec, law))
        lit = XS.exact_seats(rec.hands, rec.board, rec.n_players, rec.ghost, G.RANGES[rec.rng], uniform)
        assert row[0] == w[0] and row[1] == 0 and len(lit) == rec.n_players
        for s, (win, tie, share) in enumerate(lit):
            assert (Fraction(row[2 + 3 * s], row[0]), Fraction(row[3 + 3 * s], row[0]), Fraction(row[4 + 3 * s], UNIT * row[0])) \
                == (win, tie, share), (s, rec)
        check_invariants(G.ext_seats_row(rec, law), rec.n_players)
        assert row[2:4] == w[2:4]
    if "seats" in rec.entries:      # the all-in build walks the same record to the same row
        assert _ints(G.seats_row(rec, law)) == _ints(G.ext_seats_row(rec, law))


@pytest.mark.parametrize("law", G.LAWS)
def test_unrestricted_records_equal_the_plain_enumeration_and_the_oracle(law):
    mine = [r for r in G.grid() if "exact" in r.entries]
    assert {(r.kind, r.nb) for r in mine} == {(k, nb) for k in (0, 1, 2) for nb in G.STREETS} - {(2, 3)}
    for r in mine:
        w = _ints(G.exact_row(r, law))
        assert w == _ints(G.plain_row(r, law)[1]), r
        if r.kind == 1 or r.literal == "oracle":
            win, tie, _ = O.exact(r.hero, r.board, r.n_players, law == "uniform")
            assert abs(w[2] / w[0] - win) < ORACLE_TOL and abs(w[3] / w[0] - tie) < ORACLE_TOL, r
        assert sum(w[4:]) == w[2] + w[3]


@pytest.mark.parametrize("law", G.LAWS)
def test_all_in_preflop_rows_equal_the_plain_enumeration(law):
    """Kind 0 preflop: C(L, 5) completions, each hand scored by oracle.score_batch -- exact integer equality."""
    mine = [r for r in G.grid() if r.nb == 0]
    assert [r.n_known + 1 for r in mine] == [2, 3, 10]
    for r in mine:
        plain, ways, seats = G.enumerate_all_in(r, law)
        assert _ints(G.plain_row(r, law)[1]) == _ints(plain), r
        assert _ints(G.ways_row(r, law)) == _ints(ways), r
        assert _ints(G.seats_row(r, law)) == _ints(seats) == _ints(G.ext_seats_row(r, law)), r
        check_invariants(seats, r.n_players)


def test_the_enumerations_weights_restate_the_literal_rule():
    """exact_literal._tables on a small deck: under the reference's law a set has weight 0 when it holds the deck's
    highest card and one common weight otherwise; under the uniform law one common weight."""
    deck = [3, 8, 9, 20, 31, 40, 47]
    for k in (1, 2, 3, 5):
        ref, _ = X._tables(deck, k, False)
        assert len(set(ref.values())) == 1 and all(47 not in t for t in ref) and len(ref) == G.binom(6, k)
        uni, _ = X._tables(deck, k, True)
        assert len(set(uni.values())) == 1 and len(uni) == G.binom(7, k)
    rec = [r for r in G.grid() if "tie_ten_way_all_in" == r.name][0]     # and enumerate_all_in agrees with a walked record
    for law in G.LAWS:
        assert _ints(G.enumerate_all_in(rec, law)[2]) == _ints(G.seats_row(rec, law))
    turn = [r for r in WALKED if r.kind == 0 and r.nb == 4 and r.n_known >= 2][0]
    for law in G.LAWS:
        plain, ways, seats = G.enumerate_all_in(turn, law)
        assert _ints(ways) == _ints(G.ways_row(turn, law)) and _ints(seats) == _ints(G.seats_row(turn, law))


def test_capped_plans_give_every_owner_several_completions():
    """At MCQ_EXACT_CU = 1 and 3 (a device has more CUs than that, so the plans see the cap itself).

    A wave of kind 1 and a block of kind 2 own three completions at least on every flop record at both caps, and on every
    turn record wherever the turn has enough of them: 46 at the most, so kind 1 -- sixteen waves a block -- reaches three
    a wave at cap 1 only.  A river record has ONE completion; there only mcq_exact_kernel<true> has several units, the
    slices of its first-opponent loop.  A lane of kind 0 owns two completions on a flop only when nobody else holds cards
    (C(47, 2) = 1081 > 1024; one known hand leaves C(45, 2) = 990): the lanes' sums across completions are reached by the
    all-in preflop records, up to 1673 a lane at cap 1."""
    recs = G.grid()
    for cap in (1, 3):
        for r in recs:
            if r.kind >= 1 and r.nb == 3:
                assert G.busiest(r, "ext", cap) >= 3, (cap, r)
            if r.kind == 2 and r.nb == 4:
                assert G.busiest(r, "ext", cap) >= 3, (cap, r)
            if "exact" in r.entries and r.kind >= 1 and (r.nb == 3 or r.kind == 2):
                assert G.busiest(r, "exact", cap) >= 3, (cap, r)
            if r.kind == 0 and r.nb == 0:
                assert G.busiest(r, "ext", cap) >= 3, (cap, r)
    for r in recs:
        if r.kind == 1 and r.nb == 4:
            assert G.busiest(r, "ext", 1) >= 3, r
        if "exact" in r.entries and r.kind == 1 and r.nb == 4:
            assert G.busiest(r, "exact", 1) >= 3, r
        if r.kind == 0 and r.nb == 3:
            assert G.busiest(r, "ext", 1) == (2 if r.n_known == 0 and not r.ghost else 1), r
    assert any(r.kind == 0 and r.nb == 3 and G.busiest(r, "ext", 1) == 2 for r in recs)
    assert max(G.busiest(r, "ext", 1) for r in recs if r.nb == 0) == 1673
    # mcq_exact_kernel<true>: its largest cut of the first-opponent loop, and a walk over unit / slices, unit % slices
    river = [r for r in recs if "exact" in r.entries and r.kind == 2 and r.nb == 5][0]
    assert G.plan_exact(river, 1)[1] == 32 and G.plan_exact(river, 3)[1] == 64 and G.plan_exact(river, 256)[1] == 64
    turn = [r for r in recs if "exact" in r.entries and r.kind == 2 and r.nb == 4][0]
    assert [G.plan_exact(turn, c)[1] for c in (1, 3)] == [1, 2]
    # two jobs of kind 2 in one call: the second one's sums lie behind the first one's
    assert [r.kind for r in G.batch("ext")].count(2) >= 2
