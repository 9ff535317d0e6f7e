"""The opponents' cards read by the table's flush suit (mcq_hole_entry, hole_by_suit, McqDeckBySuit; the straight forms of
mcq_iteration_sum read them behind the table), without a GPU.  tests/hostsim_bysuit builds the lane code for the host.

* Entries.  For the base decks of queries before the flop, on the flop, the turn and the river, hero suited and off suit:
  every position x every suit, the entry {doubled rank weight, the card's tfid byte-offset bit if its suit is the one asked
  for} as McqSumHole::set and the v_perm of mcq_sum_first extract it from today's McqCard == the entry derived from the card
  by both card accessors == the entry read back from a hole table filled by put_holes, position-major and suit-major ==
  the same worked out here from the card's number.
* Rows.  2 to 10 players x 0, 3, 4, 5 table cards (tests/bysuit_cases.py), every query through the straight form the
  kernels' dispatch gives it: the cards read where they are dealt against the cards read by suit -- derived from the array of
  cards, from a position-major and from a suit-major hole table -- word for word, plain and split-pot rows, both dealing
  laws; the plain rows also against the oracle.
* The same lane code in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (hole tables of exactly
  1600 bytes at the end of their heap blocks).
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bysuit_cases
from tests import hostbuild
from tests import hostsim_bysuit as B

SEED, FQ = (1 << 44) | 0xB5017, 41
RUNS = 1041
LAWS = [(O.MODE_CTR, False), (O.MODE_CTR_UNIFORM, True)]
CELLS = bysuit_cases.cells()

# (hole, board): before the flop, flop, turn, river; hero suited and off suit
DECKS = [([48, 44], []), ([48, 45], []), ([21, 5], [30, 34, 3]), ([21, 6], [30, 34, 3]), ([0, 4], [8, 12, 16, 20]),
         ([0, 5], [51, 50, 49, 48]), ([2, 3], [28, 29, 30, 31, 32]), ([51, 47], [0, 1, 2, 3, 4])]


def one_query(hole, board, players=6, runs=1):
    return O.pack_queries(np.array([hole], np.uint8), np.array([list(board) + [255] * (5 - len(board))], np.uint8),
                          np.array([players]), runs)


def test_every_entry_of_every_base_deck():
    assert B.wave_bytes() == 1600 and B.shipped()
    w2 = [B.rank_weight2(r) for r in range(13)]
    for hole, board in DECKS:
        n, got = B.entries(one_query(hole, board))
        deck = [c for c in range(52) if c not in hole and c not in board]      # the ordered remaining deck
        assert n == len(deck) == 50 - len(board)
        want = np.zeros((B.POSITIONS, 4, 2), np.uint32)
        for p, c in enumerate(deck):
            for s in range(4):
                want[p, s] = (w2[c >> 2], (4 << (c >> 2)) if (c & 3) == s else 0)
        for k, src in enumerate(B.ENTRY_SOURCES):
            bad = np.argwhere((got[k, :n] != want[:n]).any(2))
            assert len(bad) == 0, (hole, board, src, bad[:4], got[k][tuple(bad[0])], want[tuple(bad[0])])
        # positions behind the deck's end are nobody's, but every accessor agrees on them too (the tables are written whole)
        for k in range(1, len(B.ENTRY_SOURCES)):
            assert np.array_equal(got[k], got[0]), (hole, board, B.ENTRY_SOURCES[k])
        assert (got[0][:n, :, 1] != 0).sum() == n                              # every card in exactly one suit's column


def form_of(cell):
    """the straight instantiation mcq_iterations_sum picks"""
    nopp, ndeal = cell[2] - 1, 5 - len(cell[1])
    return nopp, (ndeal if ndeal in (5, 2, 1) and nopp <= 7 else -1)


@pytest.fixture(scope="module")
def dealt_rows():
    """per (law, ways): the rows with the cards read where they are dealt -- computed once, read-only"""
    bysuit_cases.check_coverage(CELLS)
    q = bysuit_cases.pack(CELLS, RUNS, O.pack_queries)
    out = {}
    for _, uniform in LAWS:
        for ways in (False, True):
            r = np.concatenate([B.rows(q[i:i + 1], SEED, FQ + i, *form_of(c), B.DEALT, uniform=uniform, ways=ways)
                                for i, c in enumerate(CELLS)])
            r.setflags(write=False)
            out[uniform, ways] = r
    return out


@pytest.mark.parametrize("mode,uniform", LAWS, ids=["reference_law", "uniform_law"])
def test_cards_read_where_dealt_equal_the_oracle(dealt_rows, mode, uniform):
    q = bysuit_cases.pack(CELLS, RUNS, O.pack_queries)
    exp = O.run_batch(mode, np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16), SEED, first_qid=FQ, threads=8)
    assert np.array_equal(dealt_rows[uniform, False], exp)
    assert np.array_equal(dealt_rows[uniform, True][:, :13], exp)
    assert dealt_rows[uniform, True][:, 14:].any()                             # pots shared three ways and more occur
    assert exp[:, 4 + 5].sum() > 0                                             # hero wins with flushes


@pytest.mark.parametrize("accessor", [B.BY_SUIT_CARDS, B.BY_SUIT_POSITION_MAJOR, B.BY_SUIT_SUIT_MAJOR],
                         ids=["from_cards", "position_major", "suit_major"])
@pytest.mark.parametrize("ways", [False, True], ids=["plain", "split_pot"])
def test_cards_read_by_suit_give_the_same_rows(dealt_rows, accessor, ways):
    q = bysuit_cases.pack(CELLS, RUNS, O.pack_queries)
    for _, uniform in LAWS:
        want = dealt_rows[uniform, ways]
        for i, c in enumerate(CELLS):
            got = B.rows(q[i:i + 1], SEED, FQ + i, *form_of(c), accessor, uniform=uniform, ways=ways)[0]
            assert np.array_equal(got, want[i]), (c, uniform, got, want[i])


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- the table fill and every entry of a few decks, iterations of a few forms through every accessor --
    built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
    lines = hostbuild.run_sanitized("hostsim_bysuit/hs_main.cpp", "-O0", tmp_path)
    assert lines[-1].startswith("ok:"), lines
