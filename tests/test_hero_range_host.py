"""The hero-range exact enumeration's lane code (csrc/mcq_exact_hero.hpp) on the host, no GPU: its rows are the rows of the
one-record enumeration hand by hand, an independent literal walk of the reference agrees, and every refusal holds."""
import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hero_range_cases as HC
from tests import hostbuild
from tests import hostsim_exact_ext as XS
from tests import hostsim_hero_range as HS

LAWS = [0, 1]   # MCQ_LAW_REFERENCE, MCQ_LAW_UNIFORM
_rows = {}


def rows_of(name, law):
    """The host build's (rows, agg) of a case, computed once and left unchanged."""
    key = (name, law)
    if key not in _rows:
        q, x = HC.records(HC.CASES[name])
        r, a = HS.hero_range(q, x, law)
        r.setflags(write=False)
        _rows[key] = (r, a)
    return _rows[key]


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", HC.HOST_CASES)
def test_rows_are_the_one_record_rows(name, law):
    case = HC.CASES[name]
    rows, _ = rows_of(name, law)
    hands = HC.allowed_hands(case)
    assert hands
    if name == "river_all":
        assert len(hands) == 1081                      # more than one group of 1024 hero hands
    if name == "turn_one_class":
        assert len(hands) == 3                         # 77 with 7C on the table
    if name == "turn_ghost":
        assert len([i for i in range(169) if (int(HC.parts(case)[1][i >> 5]) >> (i & 31)) & 1]) >= 40
    q, x = HC.hand_records(case, hands)
    live = np.zeros(HS.ROWS, bool)
    for i, h in enumerate(hands):
        _, w = XS.exact_ext(q[i:i + 1], x[i:i + 1], uniform=bool(law))
        idx = _lib.hand_index(*h)
        live[idx] = True
        assert w[1] == 0 and w[0] > 0
        assert (rows[idx] == w).all(), (name, law, h, rows[idx], w)
    assert (rows[~live] == 0).all()


def test_the_deck_top_moves_with_the_table_and_ghost_cards():
    """AS in the deck (river_all), on the table (turn_ghost) and among the ghost cards (turn_one_class)."""
    assert HC.AS in HC.deck(HC.CASES["river_all"]) and max(HC.deck(HC.CASES["turn_ghost"])) == 50
    assert max(HC.deck(HC.CASES["turn_one_class"])) == 50
    assert any(HC.AS in h for h in HC.allowed_hands(HC.CASES["river_all"]))
    assert any(50 in h for h in HC.allowed_hands(HC.CASES["turn_ghost"]))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ["river_small", "turn_small"])
def test_literal_walk_of_the_reference(name, law):
    case = HC.CASES[name]
    rows, agg = rows_of(name, law)
    per, lit_agg = HC.literal(case, bool(law))
    assert sorted(per, key=lambda h: _lib.hand_index(*h)) == HC.allowed_hands(case)
    for h, want in per.items():
        assert HC.row_fractions(rows[_lib.hand_index(*h)]) == want, (name, law, h)
    assert int((rows[:, 0] != 0).sum()) == len(per)
    for got, want in zip(agg, lit_agg):
        assert abs(got - float(want)) <= 1e-12, (name, law, got, float(want))


def test_uniform_law_invariant_of_two_ranges():
    """Ranges A and B on one turn: every disjoint triple (h in A, g in B, table card) is a win for h, a win for g or a
    tie, seen once from each side."""
    table, a, b = ["5C", "8D", "QH", "KS"], 0.25, {"AKS", "QQ", "T9O", "76S", "KQO", "55", "A5S", "JTS"}
    ab, ba = (a, b, table, None), (b, a, table, None)
    r_ab, _ = HS.hero_range(*HC.records(ab), 1)
    r_ba, _ = HS.hero_range(*HC.records(ba), 1)
    ha, hb = HC.allowed_hands(ab), HC.allowed_hands(ba)
    triples = sum(len(HC.deck(ab)) - 4 for h in ha for g in hb if not set(h) & set(g))
    win_ab, tie_ab = int(r_ab[:, 2].sum()), int(r_ab[:, 3].sum())
    win_ba, tie_ba = int(r_ba[:, 2].sum()), int(r_ba[:, 3].sum())
    assert win_ab + win_ba + tie_ab == triples
    assert tie_ab == tie_ba
    assert int(r_ab[:, 0].sum()) == triples == int(r_ba[:, 0].sum())


@pytest.mark.parametrize("name", ["river_all", "turn_ghost", "turn_one_class", "flop_3cls"])
def test_reference_law_hero_weights(name):
    case = HC.CASES[name]
    q, x = HC.records(case)
    w = HS.hero_weights(q, x, 0)
    draw = HC.hero_draw(case, uniform=False)     # accepted ordered index pairs per hand
    top = max(HC.deck(case))
    assert {_lib.hand_index(*h): n for h, n in draw.items()} == {int(i): int(w[i]) for i in np.flatnonzero(w)}
    for h in HC.allowed_hands(case):
        assert int(w[_lib.hand_index(*h)]) == (1 if top in h else 2)
    assert sorted(np.flatnonzero(HS.hero_weights(q, x, 1))) == sorted(_lib.hand_index(*h) for h in HC.allowed_hands(case))
    assert set(HS.hero_weights(q, x, 1)) <= {0, 1}


def _refused(q, x, law=0):
    with pytest.raises(ValueError) as e:
        HS.hero_range(q, x, law)     # (checks that the outputs were left untouched)
    return str(e.value)


def test_refusals():
    case = HC.CASES["turn_ghost"]
    q, x = HC.records(case)
    HS.hero_range(q, x, 0)
    qh, xh = HC.records(case, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    assert _refused(qh, xh) == "hero is not a range"
    assert _refused(*HC.records(case, n_players=3)) == "not heads-up"
    assert _refused(*HC.records(case, n_players=1)) == "not heads-up"
    assert _refused(q, x, law=2) == "bad law"
    x2 = x.copy()
    x2["n_known"] = 1
    x2["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    q3 = q.copy()
    q3["n_players"] = 3
    assert _refused(q3, x2) == "known hands"
    q0 = _lib.pack_query_one([0, 0], [], 2, 1)
    assert _refused(q0, x) == "preflop"
    # what mcq_eval_batch_ext refuses: a table card named twice, a ghost card on the table, an empty range that is used
    qd = q.copy()
    qd["board"][0, 1] = qd["board"][0, 0]
    assert _refused(qd, x) == "invalid"
    xg = x.copy()
    xg["ghost"][0] = [q["board"][0, 0], HC.C("2C")]
    assert _refused(q, xg) == "invalid"
    for field in ("hero_range", "opp_range"):
        xe = x.copy()
        xe[field] = 0
        assert _refused(q, xe) == "invalid"
    # no allowed hero hand in the deck: 77 with three sevens gone
    assert _refused(*HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None))) == "no allowed hero hand"
    # the opponent's range cannot be dealt against AH AS
    for law in (0, 1):
        assert _refused(*HC.records(HC.UNDEALABLE), law=law) == "range cannot be dealt"


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- a river and a ghost turn, both laws -- built with AddressSanitizer and UndefinedBehaviorSanitizer and
    run as a program of its own; its aggregates are the host build's."""
    lines = hostbuild.run_sanitized("hostsim_hero_range/hs_main.cpp", "-O1", tmp_path)
    assert len(lines) == 4 and all(" rc 0," in ln for ln in lines), lines
    pairs_and_suited_aces = ["%s%s" % (r, r) for r in "23456789TJQKA"] + ["A%sS" % r for r in "23456789TJQK"]
    river = (_lib.pack_query_one([0, 0], [4, 17, 22, 35, 44], 2, 1), _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES))
    turn = (_lib.pack_query_one([0, 0], [51, 29, 10, 40], 2, 1),
            _lib.pack_query_ext(1, ghost=[0, 45], hero_range=_lib.ALL_CLASSES, opp_range=_lib.range_bits(pairs_and_suited_aces)))
    for ln, (name, rec, law) in zip(lines, [("river", river, 0), ("river", river, 1), ("turn", turn, 0), ("turn", turn, 1)]):
        rows, agg = HS.hero_range(rec[0], rec[1], law)
        assert ln.startswith("%s law %d:" % (name, law)), ln
        assert "%d hero hands, win %.9f tie %.9f" % (int((rows[:, 0] != 0).sum()), agg[0], agg[1]) in ln, (ln, agg[:2])
