"""The weighted-range-per-seat Monte-Carlo entry on the host: the lane code of mcq_ranges.hpp (tests/hostsim_ranges)
against literal Python enumerations of its law,  P(h_0, .., h_{p-1}) ~ prod_s eff_s(h_s) * [pairwise disjoint],  then the
missing table cards uniformly.  Fixed seeds, 5.5 sigma (tests/lawstats.py): a failure is a finding about the law."""
from collections import Counter

import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hostsim_ranges as H
from tests import lawstats as LS
from tests import seats_expect as SE
from tests.ranges_law import cid, hand, hidx, joint_law, literal_rows, table

UNIT = 2520


def query(board, p, runs):
    return _lib.pack_query_one([0, 0], [cid(c) for c in board], p, runs)


def dealt(hands, p):
    """hook record [runs, 2p + 5] -> Counter of the joint outcomes, each hand as (a, b) with a < b"""
    c = Counter()
    for row in hands:
        c[tuple((int(min(row[2 * s], row[2 * s + 1])), int(max(row[2 * s], row[2 * s + 1]))) for s in range(p))] += 1
    return c


def z_of(k, n, p):
    return (k / n - p) / max((p * (1.0 - p) / n) ** 0.5, 1.0 / n)


RIVER = ["2C", "7D", "9H", "JS", "KC"]
# overlapping cards on purpose (AS, AH, QD, TD appear on both sides); '9HAC' and 'KCQS' hold a table card: eff = 0
S0 = {"ASAH": 3, "ASKD": 5, "QDQH": 1, "TDTC": 7, "8C8D": 2, "9HAC": 6, "AHQD": 4, "5C6C": 1}
S1 = {"ASAD": 2, "AHKD": 7, "QDJD": 3, "TDTH": 1, "4C4D": 5, "KCQS": 4, "8C3D": 6, "ASQH": 2}
S2 = {"ASQC": 1, "4C5D": 3, "TD8D": 2, "6S6H": 7, "AHAD": 4, "3D3C": 5, "QHQS": 6}


@pytest.mark.parametrize("supports", [(S0, S1), (S0, S1, S2), ({"ASKD": 9}, S1, S2)],
                         ids=["2 seats", "3 seats", "a known hand and 2 seats"])
def test_dealt_law_is_the_joint_law(supports):
    p, n = len(supports), 200000
    tabs = np.stack([table(s) for s in supports])
    row, hands = H.run(query(RIVER, p, n), list(range(p)), tabs, 20261, 5, hands=True)
    law = joint_law(supports, RIVER)
    seen = dealt(hands, p)
    assert set(seen) <= set(law), "a deal of probability zero was dealt"
    assert len(law) > 20
    zs = [(k, seen.get(k, 0) / n, pr, z_of(seen.get(k, 0), n, pr)) for k, pr in law.items()]
    LS.check("joint law, %d seats, %d outcomes" % (p, len(law)), zs)
    assert (hands[:, 2 * p:] == [cid(c) for c in RIVER]).all()   # the table is the record's
    assert int(row[1]) > n   # overlapping supports: some trials were abandoned


def test_whole_trial_rejection_not_sequential_redraw():
    """Supports on which "redraw only the colliding seat" and the joint law differ by tens of sigma: the test can tell."""
    s0 = {"ASAH": 1, "KSKH": 1}
    s1 = {"ASAD": 1, "QSQH": 1, "TSTH": 1}   # ASAD collides with ASAH
    n = 100000
    law = joint_law((s0, s1), RIVER)
    p_joint = sum(v for k, v in law.items() if k[0] == hand("ASAH"))    # 2 / 5
    p_seq = 0.5                                                         # seat 0 first, seat 1 re-drawn from what is left
    assert p_joint == pytest.approx(0.4)
    gap = abs(p_joint - p_seq) / (p_joint * (1 - p_joint) / n) ** 0.5
    assert gap > 20
    _, hands = H.run(query(RIVER, 2, n), [0, 1], np.stack([table(s0), table(s1)]), 77, 0, hands=True)
    seen = dealt(hands, 2)
    k = sum(v for key, v in seen.items() if key[0] == hand("ASAH"))
    LS.check("P(seat 0 holds ASAH)", [("joint", k / n, p_joint, z_of(k, n, p_joint))])
    LS.check("every outcome", [(key, seen.get(key, 0) / n, pr, z_of(seen.get(key, 0), n, pr)) for key, pr in law.items()])


@pytest.mark.parametrize("board", [RIVER, RIVER[:4]], ids=["river", "turn"])
def test_rows_against_the_literal_enumeration(board):
    supports, n = (S0, S1, S2), 300000
    row = H.run(query(board, 3, n), [0, 1, 2], np.stack([table(s) for s in supports]), 31337, 2)
    SE.check_invariants(row, 3)
    seats = SE.seat_words(row)
    res = []
    for s, (pw, pt, ms, vs) in enumerate(literal_rows(supports, board)):
        res.append(("seat %d win" % s, int(seats[s, 0]) / n, pw, z_of(int(seats[s, 0]), n, pw)))
        res.append(("seat %d tie" % s, int(seats[s, 1]) / n, pt, z_of(int(seats[s, 1]), n, pt)))
        got = int(seats[s, 2]) / (UNIT * n)
        res.append(("seat %d share" % s, got, ms, (got - ms) / max((vs / n) ** 0.5, 1.0 / n)))
    LS.check("rows, %d table cards" % len(board), res)


def test_rows_are_the_recount_of_the_dealt_hands():
    """The tally itself: every seat recounted from the hook's hands with the oracle's comparison, flop, six seats."""
    n, p = 3000, 6
    wide = np.ones((1, 1326), np.uint16)
    row, hands = H.run(query(RIVER[:3], p, n), [0] * p, wide, 9, 1, hands=True)
    ks = set()
    assert np.array_equal(SE.seat_words(row), SE.recount(hands, p, ks))
    assert len(ks) >= 2
    for r in hands:
        assert len(set(int(c) for c in r)) == 2 * p + 5   # the hands and the table are disjoint
    SE.check_invariants(row, p)


def test_table_draws_are_uniform():
    """Preflop, two one-hot seats: each of the five table cards is uniform over the 48 cards left, the ace of spades -- the
    deck's highest card, which the reference's law never deals -- included."""
    n = 100000
    tabs = np.stack([table({"2C2D": 1}), table({"3C3D": 9})])
    row, hands = H.run(query([], 2, n), [0, 1], tabs, 4242, 0, hands=True)
    assert int(row[1]) == n
    left = [c for c in range(52) if c not in (0, 1, 4, 5)]
    res = []
    for pos in range(5):
        cnt = np.bincount(hands[:, 4 + pos], minlength=52)
        assert cnt[[0, 1, 4, 5]].sum() == 0
        res += [("position %d card %d" % (pos, c), cnt[c] / n, 1 / 48, z_of(int(cnt[c]), n, 1 / 48)) for c in left]
    anyp = np.bincount(hands[:, 4:].reshape(-1), minlength=52)
    res += [("card %d" % c, anyp[c] / n, 5 / 48, z_of(int(anyp[c]), n, 5 / 48)) for c in left]
    LS.check("table cards", res)
    assert anyp[51] > 0
    for r in hands[:2000]:
        assert len(set(int(c) for c in r[4:])) == 5


def test_word_to_hand_mapping():
    """t = mulhi32(word, total); the first hand in MCQ_HAND_INDEX order whose inclusive cumulative weight exceeds t."""
    g = np.random.default_rng(5)
    hands = [(a, b) for b in range(52) for a in range(b)]
    assert [hidx(h) for h in hands] == list(range(1326))
    for case in range(6):
        t = g.integers(0, 65536, 1326).astype(np.uint16)
        if case % 2:
            t[g.random(1326) < 0.9] = 0
        if case == 4:
            t[:] = 65535
        cum = np.cumsum(t.astype(np.int64))
        for w in [0, 1, 2 ** 32 - 1, 2 ** 31] + [int(x) for x in g.integers(0, 2 ** 32, 300)]:
            tt = (w * int(cum[-1])) >> 32
            want = hands[int(np.searchsorted(cum, tt, side="right"))]
            assert H.pick(t, w) == want and t[hidx(want)] > 0


def test_exact_identities():
    wide = np.ones((1, 1326), np.uint16)
    for nb, p, runs in ((0, 2, 1000), (3, 4, 777), (4, 10, 130), (5, 3, 1025)):
        row = H.run(query(RIVER[:nb], p, runs), [0] * p, wide, 1, nb)
        assert int(row[0]) == runs and int(row[1]) >= runs
        SE.check_invariants(row, p)   # sum of the shares = 2520 * runs, seats >= p zero
    # disjoint supports off the board: no trial is ever abandoned
    tabs = np.stack([table({"ASAH": 2, "KSKH": 1}), table({"QSQH": 1, "JSJH": 5}), table({"2D3D": 1})])
    row = H.run(query(RIVER[:3], 3, 5000), [0, 1, 2], tabs, 3, 0)
    assert int(row[1]) == 5000
    # a support hand on the board is re-drawn by its seat alone: still no abandoned trial
    tabs2 = np.stack([table({"ASAH": 2, "KCKH": 1}), table({"QSQH": 1, "JSJH": 5})])
    row = H.run(query(RIVER, 2, 5000), [0, 1], tabs2, 3, 0)
    assert int(row[1]) == 5000
    # one-hot tables on a full board: runs x the showdown
    one = np.stack([table({"ASAH": 1}), table({"KSKH": 9}), table({"ADAC": 65535})])
    row = H.run(query(RIVER, 3, 999), [0, 1, 2], one, 8, 0)
    s = SE.seat_words(row)
    # (table 2C 7D 9H JS KC: kings make a set; the two pairs of aces lose)
    assert [int(x) for x in s[1]] == [999, 0, 999 * UNIT] and not s[0].any() and not s[2].any() and int(row[1]) == 999
    one2 = np.stack([table({"ASAH": 1}), table({"ADAC": 3})])
    row = H.run(query(["2C", "7D", "9H", "JS", "QC"], 2, 64), [0, 1], one2, 8, 0)
    s = SE.seat_words(row)
    assert [int(x) for x in s[0]] == [0, 64, 64 * UNIT // 2] == [int(x) for x in s[1]]


def test_shared_table_or_equal_copies():
    t = table(S0)
    q = query(RIVER[:3], 3, 2000)
    a = H.run(q, [0, 0, 0], t[None, :], 11, 4)
    b = H.run(q, [0, 1, 2], np.stack([t, t, t]), 11, 4)
    c = H.run(q, [2, 0, 2], np.stack([t, table(S1), t]), 11, 4)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert not np.array_equal(a, H.run(q, [0, 0, 0], t[None, :], 11, 5))   # the query id keys the streams
    # entries at or above n_players are not read
    assert np.array_equal(a, H.run(q, [0, 0, 0, 99, 7, 7, 7, 7, 7, 7], t[None, :], 11, 4))


def test_refusals_and_the_failure_marker():
    t = table({"ASAH": 1})
    for bad in (query(RIVER[:2], 2, 10), query(RIVER[:1], 2, 10), query(RIVER, 1, 10), query(RIVER, 2, 0),
                query(["2C", "2C", "3D"], 2, 10)):
        with pytest.raises(ValueError) as e:
            H.run(bad, [0, 0], t[None, :], 1, 0)
        assert e.value.args[0] == -1
    with pytest.raises(ValueError) as e:   # a seat_table entry >= n_tables
        H.run(query(RIVER, 2, 10), [0, 1], t[None, :], 1, 0)
    assert e.value.args[0] == -1
    with pytest.raises(ValueError) as e:   # no hand clear of the table cards
        H.run(query(["AS", "7D", "9H"], 2, 10), [0, 1], np.stack([t, table({"KSKH": 1})]), 1, 0)
    assert e.value.args[0] == -1
    with pytest.raises(ValueError) as e:   # two seats one-hot on the same hand: no accepted trial
        H.run(query(RIVER, 2, 1), [0, 0], t[None, :], 1, 0)
    assert e.value.args[0] == H.FAILED
