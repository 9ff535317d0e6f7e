"""Expected rows of mcq_eval_batch_ranges_hands from code that knows nothing of the per-hand tally: the host build of the
ranges lane code (tests/hostsim_ranges) hands back every iteration's deal, and recount() recounts it per iteration with
oracle.compare, the comparison seats_expect.recount uses -> for every seat the [1326, 4] rows (runs, win, tie, share) by the
hand the seat held.  Neither the per-hand kernel nor the accumulator hook of the lane code is involved.

The cases and their expectations are computed once and shared by the host and the GPU tests."""
import functools

import numpy as np

from neuron_poker_amd import _lib
from oracle import oracle as O
from tests import hostsim_ranges as HR
from tests.ranges_law import cid

UNIT = 2520
ROWS = 1326


def hidx(a, b):
    a, b = (a, b) if a < b else (b, a)
    return b * (b - 1) // 2 + a


def recount(hands, n_players):
    """uint64 [n_players, 1326, 4]: per seat and hand it held, the iterations and the seat's win, tie, share in them,
    recounted from the dealt hands [runs, 2 n + 5] with oracle.compare."""
    out = np.zeros((n_players, ROWS, 4), np.uint64)
    for row in hands:
        table = [int(c) for c in row[2 * n_players:]]
        seven = [[int(row[2 * p]), int(row[2 * p + 1])] + table for p in range(n_players)]
        level = [0]
        for p in range(1, n_players):
            c = O.compare(seven[p], seven[level[0]])   # > 0: hand p is greater
            if c > 0:
                level = [p]
            elif c == 0:
                level.append(p)
        k = len(level)
        for p in range(n_players):
            h = hidx(seven[p][0], seven[p][1])
            out[p, h, 0] += 1
            if p in level:
                out[p, h, 1 if k == 1 else 2] += 1
                out[p, h, 3] += UNIT // k
    return out


BOARD = ["2C", "7D", "9H", "JS", "KC"]


def query(n_board, p, runs):
    return _lib.pack_query_one([0, 0], [cid(c) for c in BOARD[:n_board]], p, runs)


@functools.cache
def tables():
    """Four tables: every hand at weight 1; a third of the hands at random weights; a narrow one; a one-hot (known) hand."""
    g = np.random.default_rng(20261021)
    wide = np.ones(ROWS, np.uint16)
    third = np.where(g.random(ROWS) < 0.33, g.integers(1, 65536, ROWS), 0).astype(np.uint16)
    narrow = np.where(g.random(ROWS) < 0.06, g.integers(1, 1000, ROWS), 0).astype(np.uint16)
    known = np.zeros(ROWS, np.uint16)
    known[hidx(cid("AH"), cid("KH"))] = 9
    return np.stack([wide, third, narrow, known])


# (table cards, seats, runs, the seats' tables): every street, 2/3/6/10 seats, every run count of the issue -- the long
# ones at few seats, where the recount in Python stays short
CASES = [
    (0, 2, 1, (0, 1)), (0, 3, 17, (1, 0, 2)), (0, 6, 1024, (0, 1, 0, 1, 0, 0)), (0, 10, 1025, (0,) * 10),
    (3, 2, 16384, (1, 0)), (3, 3, 16385, (0, 2, 1)), (3, 6, 2500, (1, 0, 0, 2, 0, 1)), (3, 10, 17, (0,) * 9 + (1,)),
    (4, 2, 2500, (2, 1)), (4, 3, 1025, (3, 1, 0)), (4, 6, 1, (0,) * 6), (4, 10, 1024, (0, 1) * 5),
    (5, 2, 1025, (1, 1)), (5, 3, 2500, (1, 0, 3)), (5, 6, 17, (1, 0, 2, 0, 1, 0)), (5, 10, 2500, (0,) * 10),
]
SEED = 4711


@functools.cache
def expect(case, qid=0, seed=SEED):
    """CASES[case] as one record with query id `qid` -> (row uint64 [32] of tests/hostsim_ranges, rows per seat uint64
    [p, 1326, 4] of recount)."""
    nb, p, runs, seats = CASES[case]
    row, dealt = HR.run(query(nb, p, runs), list(seats), tables(), seed, qid, hands=True)
    return row, recount(dealt, p)


def record(case):
    """-> (query record, seat_table row uint32 [10])"""
    nb, p, runs, seats = CASES[case]
    st = np.zeros(10, np.uint32)
    st[:p] = seats
    return query(nb, p, runs), st


def check_sums(row, hands, seat):
    """contract 3: the rows of the hands add up to the seat's whole row"""
    row = [int(x) for x in np.asarray(row).view(np.uint64).reshape(32)]
    h = np.asarray(hands).view(np.uint64).reshape(ROWS, 4).astype(object).sum(0)
    assert [int(x) for x in h] == [row[0], row[2 + 3 * seat], row[3 + 3 * seat], row[4 + 3 * seat]], (h, row, seat)
