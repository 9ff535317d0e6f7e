"""The hand-against-hand matrix's lane code (csrc/mcq_exact_matrix.hpp) on the host, no GPU: the walk of the three kernels'
decomposition against an independent statement of the definition -- per table completion the oracle's scores of the live
hands, compared pairwise --, bit for bit on win, tie, total and the zero pattern; the refusals leave the outputs alone."""
from itertools import combinations

import numpy as np
import pytest

from neuron_poker_amd import _lib
from oracle import oracle as O
from tests import hostbuild
from tests import hostsim_matrix as HM
from tests import matrix_cases as MC

host_matrices = MC.host


def literal(name):
    """The definition: for every k-subset T of D, score the hands of D that miss T and count, over the pairs of hands that
    share no card, who is strictly above whom and who is level."""
    board = MC.CASES[name][0]
    d, hs = MC.deck(name), np.array(MC.hands(name), np.uint8)
    idx = np.array([_lib.hand_index(a, b) for a, b in hs])
    apart = ((hs[:, None, 0] != hs[None, :, 0]) & (hs[:, None, 0] != hs[None, :, 1]) &
             (hs[:, None, 1] != hs[None, :, 0]) & (hs[:, None, 1] != hs[None, :, 1]))
    k, nb = 5 - len(board), len(board)
    win, tie = np.zeros((len(hs), len(hs)), np.uint32), np.zeros((len(hs), len(hs)), np.uint32)
    n_t = 0
    for t in combinations(d, k):
        live = np.flatnonzero(~np.isin(hs, t).any(1))
        cards = np.empty((len(live), 7), np.uint8)
        cards[:, :2] = hs[live]
        cards[:, 2:2 + nb] = board
        cards[:, 2 + nb:] = t
        s = O.score_batch(cards)
        ok = apart[np.ix_(live, live)]
        win[np.ix_(live, live)] += (s[:, None] > s[None, :]) & ok
        tie[np.ix_(live, live)] += (s[:, None] == s[None, :]) & ok
        n_t += 1
    full_w, full_t = np.zeros((MC.ROWS, MC.ROWS), np.uint16), np.zeros((MC.ROWS, MC.ROWS), np.uint16)
    full_w[np.ix_(idx, idx)] = win
    full_t[np.ix_(idx, idx)] = tie
    pairs = np.flatnonzero(apart.ravel())
    totals = (win + win.T + tie).ravel()[pairs]
    assert totals.min() == totals.max()
    return full_w, full_t, int(totals[0]), n_t


@pytest.mark.parametrize("name", MC.HOST_CASES)
def test_lane_code_is_the_definition(name):
    win, tie, total = host_matrices(name)
    want_w, want_t, want_total, n_t = literal(name)
    d = len(MC.deck(name))
    k = 5 - len(MC.CASES[name][0])
    assert n_t == len(list(combinations(range(d), k)))
    MC.check_shape(name, win, tie, total)
    assert total == want_total
    assert np.array_equal(win, want_w) and np.array_equal(tie, want_t), name
    assert np.array_equal(win == 0, want_w == 0) and np.array_equal(tie == 0, want_t == 0)
    MC.check_structure(name, win, tie, total)


def test_without_tie_the_win_matrix_is_the_same():
    win, _, total = host_matrices("turn_dead2")
    got, none, got_total = HM.matrix(MC.record("turn_dead2"), want_tie=False)
    assert none is None and got_total == total and np.array_equal(got, win)


def test_dead_cards_and_table_order_do_not_change_a_pair_of_hands_beyond_its_total():
    """A river has no card to come: a dead card only empties the rows and columns of the hands that hold it, and the order
    in which the table cards are given changes nothing."""
    win, tie, _ = host_matrices("river")
    board = MC.CASES["river"][0]
    gone = MC.C("2C", "KD")
    w2, t2, total = HM.matrix(_lib.pack_matrix_query(board[::-1], gone))
    keep = np.ones(MC.ROWS, bool)
    for h in MC.hands("river"):
        if set(h) & set(gone):
            keep[_lib.hand_index(*h)] = False
    m = keep[:, None] & keep[None, :]
    assert total == 1 and np.array_equal(w2[m], win[m]) and np.array_equal(t2[m], tie[m])
    assert not w2[~m].any() and not t2[~m].any()


def _refused(q, **kw):
    with pytest.raises(ValueError) as e:
        HM.matrix(q, **kw)          # (checks that the sentinel-filled outputs were left untouched)
    return str(e.value)


def test_refusals():
    board, dead = MC.CASES["turn_dead2"][:2]
    good = _lib.pack_matrix_query(board, dead)
    HM.matrix(good)
    assert _refused(good, want_win=False) == "no win matrix"
    for nb in (0, 1, 2):
        assert _refused(_lib.pack_matrix_query(board[:nb], dead)) == "street"
    q = good.copy()
    q["n_board"] = 6
    assert _refused(q) == "street"
    for i in (0, 1):
        q = good.copy()
        q["reserved"][0, i] = 1
        assert _refused(q) == "reserved bytes"
    for bit in (52, 63):
        q = good.copy()
        q["dead"] |= np.uint64(1 << bit)
        assert _refused(q) == "mask bits"
    q = good.copy()
    q["board"][0, 3] = 52
    assert _refused(q) == "card out of range"
    q = good.copy()
    q["board"][0, 3] = q["board"][0, 0]
    assert _refused(q) == "table card twice"
    assert _refused(_lib.pack_matrix_query(board, dead + [board[2]])) == "table card dead"
    assert _refused(_lib.pack_matrix_query(*MC.REFUSED_SHORT)) == "too few cards"       # L = 4, k = 2
    ok = good.copy()
    ok["board"][0, 4] = 255                                     # (the unused slot is not read)
    assert np.array_equal(HM.matrix(ok)[0], HM.matrix(good)[0])
    # L - 4 == k is the smallest deck that is enumerated: one completion per pair of hands
    edge = _lib.pack_matrix_query(MC.CASES["flop_tiny"][0], MC.CASES["flop_tiny"][1])
    assert HM.matrix(edge)[2] == 1


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- a river, a turn with two dead cards, a flop with six cards left and a refused record -- built with
    AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own; its sums are the host build's."""
    lines = hostbuild.run_sanitized("hostsim_matrix/hs_main.cpp", "-O1", tmp_path)
    assert len(lines) == 4, lines
    flop = [50, 46, 21]
    lowest = [c for c in range(52) if c not in flop]
    for i, (board, dead) in enumerate([([4, 17, 22, 35, 44], []), ([51, 29, 10, 40], [0, 45]), (flop, lowest[:43])]):
        win, tie, total = HM.matrix(_lib.pack_matrix_query(board, dead))
        assert lines[i] == "case %d: rc 0, total %d, win %d, tie %d" % (i, total, int(win.sum(dtype=np.uint64)),
                                                                        int(tie.sum(dtype=np.uint64))), lines[i]
    assert lines[3].startswith("case 3: rc 7,"), lines[3]                       # MCQ_XM_SHORT
    assert _refused(_lib.pack_matrix_query(flop, lowest[:45])) == "too few cards"
