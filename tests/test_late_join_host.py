"""The late join of an opponent pair (mcq_iteration_sum: a pair's hand is put together behind the NEXT pair's reads, the
last pair's behind the table's draws) in every instantiation that has it, without a GPU.

tests/hostsim_join builds mcq_iteration_sum for the host with the template arguments named by the caller.  A cell is one
instantiation: 1 to 7 opponents x 5, 2, 1 table cards to come or a run-time count, 8 and 9 opponents with a run-time
count, and the general form (both counts at run time), which keeps the old order -- 31 cells, each with both accumulators
and under both dealing laws.  Per cell 64 seeded random states (hero and table drawn from a shuffled deck; where a count
is a run-time one the states go through every value it can take) of 256 iterations each: 16 streams, so every lane
function runs its 16 iterations.

* plain rows == the oracle's CTR mode, all thirteen words (runs, passes, win, tie, by_type);
* split-pot rows == tests/ways_expect.py: the oracle's tallies and a recount of its per-iteration trace.

A host compiler sees the same source text -- the `if constexpr` paths, the pending pair, the index of the hand a pair
joins -- but not the empty asm that holds the join in place on the device: tests/test_late_join_gpu.py covers that.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim_join, ways_expect

SEED, FQ = (1 << 43) | 0x10137, 11
STATES, RUNS = 64, 256
CELLS = [(n, d) for n in range(1, 8) for d in (5, 2, 1, -1)] + [(8, -1), (9, -1), (-1, -1)]
BOARDS = (5, 4, 3, 0)   # table cards of a state where the cards to come are counted at run time
LAWS = [(O.MODE_CTR, False), (O.MODE_CTR_UNIFORM, True)]


def cell_states(ci):
    """-> (hole [64, 2], board [64, 5] with 255 = absent, n_players [64]) of cell ci"""
    nopp, ndeal = CELLS[ci]
    rng = np.random.RandomState(1000 + ci)
    hole, board, npl = [], [], []
    for i in range(STATES):
        deck = rng.permutation(52)
        nb = 5 - ndeal if ndeal >= 0 else BOARDS[i % 4]
        hole.append(deck[:2])
        board.append(list(deck[2:2 + nb]) + [255] * (5 - nb))
        npl.append(nopp + 1 if nopp >= 0 else 1 + (i // 4) % 10)   # the general form: hero alone up to ten players
    return np.array(hole, np.uint8), np.array(board, np.uint8), np.array(npl)


def cell_queries(ci):
    hole, board, npl = cell_states(ci)
    return O.pack_queries(hole, board, npl, RUNS)


def all_queries():
    return np.concatenate([np.ascontiguousarray(cell_queries(ci), np.uint8).reshape(-1, 16) for ci in range(len(CELLS))])


@pytest.fixture(scope="module")
def want():
    """the oracle's rows of every cell's states, per law: computed once, read-only"""
    q = all_queries()
    out = {}
    for mode, _ in LAWS:
        w = O.run_batch(mode, q, SEED, first_qid=FQ, threads=8)
        w.setflags(write=False)
        out[mode] = w
    return out


def test_cells_are_what_they_claim():
    assert len(CELLS) == 31 and len(set(CELLS)) == 31
    q = all_queries()
    assert len(q) == 31 * STATES
    for ci, (nopp, ndeal) in enumerate(CELLS):
        rows = q[ci * STATES:(ci + 1) * STATES]
        assert len({bytes(r[:7]) for r in rows}) >= STATES - 8    # random states: before the flop two may be the same hand
        if nopp >= 0:
            assert (rows[:, 8] == nopp + 1).all()
        else:
            assert set(rows[:, 8].tolist()) == set(range(1, 11))
        if ndeal >= 0:
            assert (rows[:, 7] == 5 - ndeal).all()
        else:
            assert set(rows[:, 7].tolist()) == {0, 3, 4, 5}


@pytest.mark.parametrize("mode,uniform", LAWS, ids=["reference_law", "uniform_law"])
def test_plain_rows_equal_the_oracle(want, mode, uniform):
    for ci, (nopp, ndeal) in enumerate(CELLS):
        got = hostsim_join.rows(cell_queries(ci), SEED, FQ + ci * STATES, nopp, ndeal, uniform=uniform)
        exp = want[mode][ci * STATES:(ci + 1) * STATES]
        assert int(got[:, 0].sum()) == STATES * RUNS
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, ((nopp, ndeal), bad[:4], got[bad[:2]], exp[bad[:2]])


@pytest.mark.parametrize("mode,uniform", LAWS, ids=["reference_law", "uniform_law"])
def test_split_pot_rows_equal_the_trace(want, mode, uniform):
    seen = np.zeros(9, np.uint64)
    for ci, (nopp, ndeal) in enumerate(CELLS):
        hole, board, npl = cell_states(ci)
        got = hostsim_join.rows(cell_queries(ci), SEED, FQ + ci * STATES, nopp, ndeal, uniform=uniform, ways=True)
        assert np.array_equal(got[:, :13], want[mode][ci * STATES:(ci + 1) * STATES]), (nopp, ndeal)
        for i in range(STATES):
            b = [int(c) for c in board[i] if c != 255]
            exp = ways_expect.expected_row_fast(mode, [int(c) for c in hole[i]], b, int(npl[i]), RUNS, SEED,
                                                FQ + ci * STATES + i)
            assert np.array_equal(got[i], exp), ((nopp, ndeal), i, got[i], exp)
        seen += got[:, 13:].sum(0)
    assert int((seen != 0).sum()) >= 3, seen   # pots shared two, three and more ways occur


def test_an_instantiation_refuses_another_query():
    q = cell_queries(CELLS.index((3, 2)))[:1]
    with pytest.raises(ValueError):
        hostsim_join.rows(q, SEED, FQ, 4, 2)
    with pytest.raises(ValueError):
        hostsim_join.rows(q, SEED, FQ, 3, 5)
    with pytest.raises(ValueError):
        hostsim_join.rows(q, SEED, FQ, 8, 2)    # eight opponents: only the run-time count is instantiated
