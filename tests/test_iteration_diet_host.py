"""The plain path's iteration with its trimmed forms -- rank sums kept doubled, hole inserts by addition, the flush-suit
selector without compares, an empty starting table when five cards are dealt -- against the oracle's CTR mode, all thirteen
words of a row, without a GPU: a host build of mcq_iterations (tests/hostsim_diet) in both forms, the straight-line one the
bulk kernel runs and the general one.

* 1 to 9 opponents x 0, 3, 4, 5 table cards, 64 streams of 16 iterations each: nine opponents fill all five hole registers
  and every slot of them, and five cards to come fill the table's own register.
* Hand-picked states: four aces and three kings (the largest rank sum, 15 651 518 doubled), the wheel, a table that gives
  each of the four suits its flush and one that gives none -- as five known cards and as a flop with two to come.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim_diet

SEED, FQ = (1 << 41) | 0xD1E7, 5
RUNS = 64 * 16
BOARD = ["9H", "TH", "2S", "2D", "KC"]
HANDS = [["AS", "AD"], ["7C", "3H"], ["KH", "QH"], ["5D", "6D"]]
SUITS = "CDHS"


def pack(cells):
    """cells: (hero, board, n_players)"""
    hole = np.array([[O.card_id(c) for c in h] for h, _, _ in cells], np.uint8)
    board = np.array([[O.card_id(c) for c in b] + [255] * (5 - len(b)) for _, b, _ in cells], np.uint8)
    return O.pack_queries(hole, board, np.array([p for _, _, p in cells]), RUNS)


def host_rows(q, straight):
    L = hostsim_diet.lib()
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 16)
    out = np.zeros((len(q), 13), np.uint64)
    for i in range(len(q)):
        rec = q[i].copy()
        assert L.hs_diet_run(rec.ctypes.data_as(C.c_void_p), SEED, FQ + i, straight, out[i].ctypes.data_as(C.c_void_p)) == 0
    return out


GRID = [(HANDS[(n_opp + nb) % 4], BOARD[:nb], n_opp + 1) for n_opp in range(1, 10) for nb in (0, 3, 4, 5)]


def picked():
    cells = [(["AS", "AH"], ["AD", "AC", "KS", "KH", "KD"], 3),          # four aces + three kings: the largest sum
             (["AS", "2H"], ["3D", "4C", "5S", "9H", "KD"], 3),          # the wheel
             (["AS", "2H"], ["3D", "4C", "5S"], 3)]
    for s in SUITS:                                                      # a flush of every suit: made, and two to come
        others = [x for x in SUITS if x != s]
        cells.append((["A" + s, "4" + s], ["2" + s, "7" + s, "J" + s, "9" + others[0], "K" + others[1]], 4))
        cells.append((["A" + s, "4" + s], ["2" + s, "7" + s, "J" + s], 4))
        cells.append((["A" + others[0], "4" + others[1]], ["2" + s, "7" + s, "J" + s, "Q" + s, "K" + others[2]], 6))
    cells.append((["AS", "4H"], ["2C", "7D", "JH", "9S", "KC"], 4))      # no suit three times: no flush for anyone
    cells.append((["AS", "4H"], ["2C", "7D", "JH"], 4))
    return cells


@pytest.fixture(scope="module")
def want():
    return {"grid": O.run_batch(O.MODE_CTR, pack(GRID), SEED, first_qid=FQ, threads=8),
            "picked": O.run_batch(O.MODE_CTR, pack(picked()), SEED, first_qid=FQ, threads=8)}


def test_grid_has_every_cell():
    q = np.ascontiguousarray(pack(GRID), np.uint8).reshape(-1, 16)
    assert len(q) == 36 and len({(int(r[8]), int(r[7])) for r in q}) == 36


@pytest.mark.parametrize("straight", [1, 0], ids=["straight", "general"])
def test_one_to_nine_opponents_every_street(want, straight):
    got = host_rows(pack(GRID), straight)
    assert int(got[:, 0].sum()) == 36 * RUNS
    for i, cell in enumerate(GRID):
        assert np.array_equal(got[i], want["grid"][i]), (cell, got[i], want["grid"][i])


@pytest.mark.parametrize("straight", [1, 0], ids=["straight", "general"])
def test_hand_picked_states(want, straight):
    cells = picked()
    got = host_rows(pack(cells), straight)
    for i, cell in enumerate(cells):
        assert np.array_equal(got[i], want["picked"][i]), (cell, got[i], want["picked"][i])
    quads_full = got[0]
    assert int(quads_full[2] + quads_full[3]) == RUNS and int(quads_full[4 + 7]) == RUNS   # four aces: hero never loses


def test_doubled_sums_and_selector():
    L = hostsim_diet.lib()
    sums = [L.hs_diet_card_sum(c) for c in range(52)]
    assert all(sums[c] == sums[c & ~3] and sums[c] % 2 == 0 for c in range(52))
    assert 4 * sums[48] + 3 * sums[44] == 15651518 < 1 << 24
    for s, suit in enumerate(SUITS):                                     # three to five cards of one suit: its half-word
        for n in (3, 4, 5):
            cards = [4 * r + s for r in range(n)] + [4 * (8 + k) + (s + 1 + k) % 4 for k in range(5 - n)]
            b = np.array(cards, np.uint8)
            assert L.hs_diet_psel(b.ctypes.data_as(C.c_void_p), 5) == 0x0C0C0100 + 0x0202 * s, (suit, n)
    for cards in ([], [0, 5, 10], [0, 4, 9, 13, 18], [3, 7, 10, 14, 17]):  # no suit three times: the clubs' field
        b = np.array(cards + [0], np.uint8)
        assert L.hs_diet_psel(b.ctypes.data_as(C.c_void_p), len(cards)) == 0x0C0C0100, cards
