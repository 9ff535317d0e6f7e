"""The plain kernels with the single-hole step in their dealing (mcq_hole_pair: opponent draws J = 1, 5, 9 and table draw
K = 1 as one compare of the two draws) against the oracle, bit for bit.

One batch: 2 to 10 players x 0, 3, 4, 5 table cards x runs 1, 15, 16, 17, 1023, 1024, 1025, 2049 -- a lone lane, a lane's
stream one short, whole and one over, a task one short, whole and one over, two whole tasks and a one-lane tail -- 288
queries, and behind them one 6-max query of 257 tasks less three iterations.  A query of more than 256 tasks keeps the
host from cutting the tasks of the batch, and one of more than eight from taking the one-launch path, so the whole batch
runs in the unsplit bulk kernel (mcq_eval_kernel<MCQ_MODE_PHILOX, false, false>); eval_batch_ways sends the same batch
through the split-pot instance (<MCQ_MODE_PHILOX, false, true>), whose rows are checked in their plain thirteen words and
by tie == sum(tie_ways).  Without the long query the 288 take the one-launch kernel (the general form of the lane code).
Parity mode's mcq_iterations_replay4 shares the lane code: one small batch of 3 and 6 players on every street against the
oracle's MT mode.
"""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED, FQ = (1 << 43) | 0x5EA15, 7
MT_SEED = 20241
PLAYERS, STREETS = tuple(range(2, 11)), (0, 3, 4, 5)
RUNS = (1, 15, 16, 17, 1023, 1024, 1025, 2049)
LONG_RUNS = 257 * 1024 - 3
BOARD = ["4C", "JD", "JS", "8H", "AC"]
HANDS = [["QS", "QD"], ["2C", "7H"], ["AH", "KH"], ["9C", "TC"], ["3S", "3H"]]


def batch(with_long=True):
    hole, board, npl, runs = [], [], [], []
    for p in PLAYERS:
        for nb in STREETS:
            for k, r in enumerate(RUNS):
                hole.append([npa.card_id(c) for c in HANDS[(2 * p + nb + k) % 5]])
                board.append([npa.card_id(c) for c in BOARD[:nb]] + [255] * (5 - nb))
                npl.append(p)
                runs.append(r)
    if with_long:
        hole.append([npa.card_id(c) for c in HANDS[2]])
        board.append([255] * 5)
        npl.append(6)
        runs.append(LONG_RUNS)
    return npa.pack_queries(hole, board, npl, runs)


def parity_batch():
    hole, board, npl, runs = [], [], [], []
    for p in (3, 6):
        for nb in STREETS:
            for r in (17, 1025):
                hole.append([npa.card_id(c) for c in HANDS[(p + nb) % 5]])
                board.append([npa.card_id(c) for c in BOARD[:nb]] + [255] * (5 - nb))
                npl.append(p)
                runs.append(r)
    return npa.pack_queries(hole, board, npl, runs)


def raw16(q):
    return q.view(np.uint8).reshape(-1, 16)


def u64(r, words=13):
    return np.asarray(r).view(np.uint64).reshape(-1, words)


@pytest.fixture(scope="module")
def want():
    w = O.run_batch(O.MODE_CTR, raw16(batch()), SEED, first_qid=FQ, threads=16)
    w.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def test_batch_has_every_cell():
    q = raw16(batch())
    cells = {(int(r[8]), int(r[7]), int(r[12:16].view("<u4")[0])) for r in q[:-1]}
    assert len(q) == 289 and len(cells) == 288
    tasks = [(int(r[12:16].view("<u4")[0]) + 1023) // 1024 for r in q]
    assert max(tasks) == 257 and max(tasks[:-1]) <= 8   # the last query alone keeps the batch in the unsplit bulk kernel


def test_unsplit_bulk_kernel(eng, want):
    got = u64(eng.eval_batch(batch(), SEED, first_query_id=FQ))
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (bad[:8], raw16(batch())[bad[:4]], got[bad[:2]], want[bad[:2]])


def test_unsplit_bulk_kernel_split_pot_rows(eng, want):
    rows = u64(eng.eval_batch_ways(batch(), SEED, first_query_id=FQ), 22)
    bad = np.flatnonzero((rows[:, :13] != want).any(1))
    assert len(bad) == 0, (bad[:8], rows[bad[:2]], want[bad[:2]])
    assert np.array_equal(rows[:, 13:].sum(1), rows[:, 3])   # tie = sum of tie_ways


def test_one_launch_kernel(eng, want):
    got = u64(eng.eval_batch(batch(with_long=False), SEED, first_query_id=FQ))
    assert np.array_equal(got, want[:-1])


def test_parity_mode_three_and_six_players(eng):
    q = parity_batch()
    assert {(int(r[8]), int(r[7])) for r in raw16(q)} == {(p, nb) for p in (3, 6) for nb in STREETS}
    w = O.run_batch(O.MODE_MT, raw16(q), MT_SEED, first_qid=FQ, threads=16)
    got = u64(eng.eval_batch(q, MT_SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
    assert np.array_equal(got, w)
