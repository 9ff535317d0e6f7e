"""The table cards' position arithmetic (mcq_draw_table) against Python's list.pop on short decks and, together with the
opponents' deal, against the reference's recorded deals on the full deck; and the iteration through the kernels' deck
accessor (McqDeckSplit) against the array-of-cards accessor (McqDeckAoS).  No GPU."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim_deck

G = os.path.join(os.path.dirname(__file__), "golden")


def _sequences(length, n):
    """every sequence of n indices a deck of `length` cards allows: r_k < length - k (the uniform law; the reference
    law's r_k < length - k - 1 is the subset without the last index)"""
    return np.array(list(itertools.product(*[range(length - k) for k in range(n)])), np.uint8).reshape(-1, n)


@pytest.mark.parametrize("length", range(6, 13))
def test_unpop_equals_list_pop(length):
    L = hostsim_deck.lib()
    for n in range(1, 6):
        seq = _sequences(length, n)
        pos = np.zeros_like(seq)
        L.hs_unpop_many(seq.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint64(len(seq)), pos.ctypes.data_as(C.c_void_p))
        reference_law = uniform_law = 0
        for row, got in zip(seq.tolist(), pos.tolist()):
            deck = list(range(length))
            want = [deck.pop(r) for r in row]   # the deck is its own index: the card IS the position
            assert got == want, (length, row)
            uniform_law += 1
            reference_law += all(r < length - k - 1 for k, r in enumerate(row))
        assert 0 < reference_law < uniform_law


def _traces():
    z = np.load(os.path.join(G, "deal_traces.npz"))
    return [(m, z["hands_%d" % i]) for i, m in enumerate(json.loads(str(z["meta"])))]


def test_traces_cover_the_cells_the_issue_names():
    cells = {(m["n_players"], len(m["board"])) for m, _ in _traces()}
    assert {2, 6, 10} <= {p for p, _ in cells} and {0, 3, 4, 5} == {b for _, b in cells}


@pytest.mark.parametrize("which", range(7))
def test_full_deck_deal_equals_the_committed_traces(which):
    """The reference's recorded deals on the full deck: every dealt card's index in the list as list.pop left it is fed
    to the lane code's dealing (mcq_draw_opp for the opponents, then mcq_draw_table: the position p among the table's own holes plus the
    frozen count against the opponents' holes), and the base position it returns must hold that card."""
    m, hands = _traces()[which]
    n_opp, n_board = m["n_players"] - 1, len(m["board"])
    n_deal, D = 5 - n_board, 2 * (m["n_players"] - 1) + 5 - n_board
    known = [O.card_id(c) for c in m["hero"] + m["board"]]
    base = [c for c in range(52) if c not in known]   # the ordered remaining deck = the kernels' base table
    draws = np.zeros((len(hands), max(D, 1)), np.uint8)
    cards = np.zeros((len(hands), max(D, 1)), np.uint8)
    for it, h in enumerate(hands.tolist()):
        assert h[0][:2] == known[:2] and h[0][2:2 + n_board] == known[2:]
        deck = list(base)
        dealt = [c for p in range(1, n_opp + 1) for c in h[p][:2]] + h[0][2 + n_board:]
        for k, c in enumerate(dealt):
            draws[it, k] = deck.index(c)
            deck.pop(draws[it, k])
            cards[it, k] = c
    pos = np.zeros_like(draws)
    if D:
        hostsim_deck.lib().hs_deal_many(C.c_uint32(n_opp), C.c_uint32(n_deal), draws.ctypes.data_as(C.c_void_p),
                                        C.c_uint64(len(hands)), pos.ctypes.data_as(C.c_void_p))
        assert pos.max() < len(base)
        assert np.array_equal(np.array(base, np.uint8)[pos], cards)


def _query(hole, board, n_players, runs):
    q = np.zeros(16, np.uint8)
    q[0:2] = hole
    q[2:2 + len(board)] = board
    q[7] = len(board)
    q[8] = n_players
    q[12:16] = np.frombuffer(np.uint32(runs).tobytes(), np.uint8)
    return q


BOARDS = {0: [], 3: [7, 22, 45], 4: [7, 22, 45, 30], 5: [7, 22, 45, 30, 1]}


@pytest.mark.parametrize("n_board", [0, 3, 4, 5])
@pytest.mark.parametrize("n_players", range(2, 11))
def test_split_deck_equals_aos_deck(n_players, n_board):
    L = hostsim_deck.lib()
    q = _query([48, 49], BOARDS[n_board], n_players, 300)   # aces: every cell counts wins
    for law in (0, 1):
        for ways in (0, 1):
            for general in (0, 1):
                got = L.hs_deck_both(q.ctypes.data_as(C.c_void_p), C.c_uint64(20240229), C.c_uint64(n_players * 8 + n_board),
                                     law, ways, general)
                assert got > 0, (n_players, n_board, law, ways, general, got)
