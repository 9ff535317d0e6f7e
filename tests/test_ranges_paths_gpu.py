"""The parts of mcq_eval_batch_ranges that exist only in mcq_kernels.hip -- the parallel table scan, the decision what a
block stages in LDS, the chunked cost prefix -- bit for bit against the host build of the lane code (tests/hostsim_ranges,
which prepares its tables with the serial mcq_ranges_prefix and knows neither blocks nor staging).  Which path ran cannot
be observed from outside: every docstring states which path its shape takes, and tests/test_stage_host.py asks the kernel's
own rule (csrc/mcq_stage.hpp) the same of the same constructions (tests/ranges_paths.py).  A sample of every
batch is sent again record by record at the matching first_query_id, where a record is alone in its block."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import neuron_poker_amd as npa
from tests import hostsim_ranges as H
from tests import seats_expect as SE
from tests.ranges_paths import BOARD, STREETS, THRESHOLD_SHAPES, batch, mixed_batch, narrow_tables, threshold_shape

pytestmark = pytest.mark.gpu
SEED = 20261021
FULL = 65535


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_one_block():
    """A context whose sliced launches are ONE block (MCQ_GRID_CAP is read when the context is made)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("MCQ_GRID_CAP", "1")
    try:
        e = npa.Engine(0)
    finally:
        mp.undo()
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def check(e, recs, tables, qid, alone):
    """The batch equals the host build row by row; rows `alone` equal the same record sent on its own."""
    q, seat_table = batch(recs)

    def host(i):
        return H.run(q[i:i + 1], seat_table[i, :len(recs[i][1])], tables, SEED, qid + i)
    first = host(0)   # (builds and loads the host library; the calls after it are independent and leave the interpreter lock)
    with ThreadPoolExecutor(8) as pool:
        exp = np.stack([first] + list(pool.map(host, range(1, len(recs)))))
    # (CPU) before relying on a shape: the host build alone stays far below the trial bound
    assert all(int(r[1]) < 1000 * int(r[0]) and int(r[0]) == rec[2] for r, rec in zip(exp, recs))
    got = w32(e.eval_batch_ranges(q, seat_table, tables, SEED, first_query_id=qid))
    bad = [i for i in range(len(recs)) if not np.array_equal(got[i], exp[i])]
    assert not bad, ("rows that differ from the host build", bad[:10], [recs[i] for i in bad[:3]])
    for i in alone:
        one = w32(e.eval_batch_ranges(q[i:i + 1], seat_table[i:i + 1], tables, SEED, first_query_id=qid + i))
        assert np.array_equal(one[0], exp[i]), (i, recs[i])
    for r, rec in zip(got, recs):
        SE.check_invariants(r, len(rec[1]))
    return got


# ------------------------------------------------------------------------------------------------------- the table scan
def scan_tables():
    t = np.zeros((8, 1326), np.uint16)
    t[0] = FULL                                   # the stated bound of the total: 1326 * 65535 = 86 899 410 < 2^27
    t[1, 0] = 5                                   # one entry at index 0: a known hand, nnz = 1, last = 0
    t[2, 1325] = 9                                # one entry at index 1325: the last thread that holds hands, its last hand
    t[3, [0, 1325]] = [3, 4]                      # the two ends: everything between them is a run of equal sums
    t[4, 1320:1326] = [1, 2, 3, 4, 5, FULL]       # thread 220 only, six hands of 1326 = 221 * 6
    t[5, [383, 384, 767, 768, 1151, 1152]] = [7, 1, FULL, 2, 3, FULL]   # lane 63 of a wave and lane 0 of the next
    t[6, 1::2] = FULL                             # alternating 0 and 65535
    t[7] = FULL
    t[7, 700] = 1                                 # one entry of 1 among 65535: the scan must not lose a unit
    return t


def test_table_scan_shapes():
    """(CPU) what the shapes are about: six hands per thread, 64 threads per wave, the sums of the host form."""
    t = scan_tables()
    assert int(t[0].astype(np.int64).sum()) == 86899410 and int(t[7].astype(np.int64).sum()) == 86899410 - 65534
    assert 1320 // 6 == 1325 // 6 == 220 and 220 < 256
    for i in (383, 767, 1151):   # hand i is the last of lane 63's, hand i + 1 the first of the next wave's lane 0
        assert (i // 6) % 64 == 63 and ((i + 1) // 6) % 64 == 0
    hands = [(a, b) for b in range(52) for a in range(b)]   # MCQ_HAND_INDEX order
    assert not {c for tab in t[1:6] for i in np.nonzero(tab)[0] for c in hands[i]} & set(BOARD)   # named hands clear of the table


def test_table_scan_against_the_serial_prefix(eng):
    """mcq_ranges_tables_kernel, one block per table: 256 threads of six consecutive hands, a shuffle scan in each of the
    four waves, the waves' totals through LDS, nnz and last by atomicAdd / atomicMax.  Every draw of the evaluation
    searches the prepared sums, so a sum that is off by one unit anywhere moves hands and the rows differ from the host
    build, which sums serially.  Flop records of 2 and 3 seats, 64 and 1025 runs; each special table sits on one seat
    (two seats on a table whose hands all share a card would block each other), the wide ones on the others.  Tables
    1 and 2 have one entry: their seats are known hands, which is what nnz and last exist for."""
    t = scan_tables()
    recs = []
    for k in range(8):
        recs.append((3, [k, 0], 64))
        recs.append((3, [6, k, 7], 1025))
    recs.append((3, [1, 2], 1025))        # two known hands: nothing is drawn
    recs.append((3, [3, 4, 5], 64))       # three narrow tables whose hands can all be disjoint
    got = check(eng, recs, t, 3000, alone=[0, 3, 8, 11, 16, 17])
    assert int(got[16, 1]) == 1025


# ------------------------------------------------------------------------------------------- what a block stages in LDS
@pytest.mark.parametrize("shape", THRESHOLD_SHAPES)
def test_staging_thresholds_in_one_block(eng_one_block, shape):
    """One block sees every record of the call.  It stages when its records are at most MCQ_RG_STAGE_QUERIES = 32 and
    name at most MCQ_RG_STAGE_TABLES = 6 distinct tables, tables with one entry not counted:
      32 records, 6 tables                     -> staged, all six slots of s_cum in use;
      32 records, 7 tables                     -> the seventh table does not fit: every draw reads HBM;
      33 records, 6 tables                     -> one record too many: HBM;
      32 records, 6 tables and 4 known hands   -> ten distinct tables, four of them known hands: staged;
      known hands only                         -> no table to stage, no draw at all: passes == runs."""
    recs, tables = threshold_shape(shape)
    got = check(eng_one_block, recs, tables, 4000, alone=[0, 5, len(recs) - 1])
    if shape == "known hands only":
        assert all(int(r[0]) == int(r[1]) for r in got)


# ------------------------------------------------------------------------------------------------------- mixed blocks
def test_blocks_that_stage_beside_blocks_that_do_not(eng):
    """48 flop records of 2500 runs (three wave tasks each) on the default grid: 144 tasks, one block of four waves per
    task.  Records 0..23 (2 to 6 seats) name tables 0..5 only, records 24..47 seat ten players on ten distinct full-width
    tables each.  A block whose piece of the cost axis lies inside the first 24 records finds at most six tables and
    stages them; one inside the last 24 finds ten and reads HBM; the block whose piece holds the end of record 23 and the
    start of record 24 names fifteen, and its waves run BOTH kinds of record from HBM.  The cost axis is cut by price
    (seats, street, estimated trials), not by record: with the host's prices for these tables blocks 0..67 lie among the
    first 24 records (one to three records each, so fewer than six tables are staged in most), block 68 holds the change
    and blocks 69..143 lie among the last 24."""
    recs, tables = mixed_batch()
    check(eng, recs, tables, 5000, alone=[0, 23, 24, 47])


# ----------------------------------------------------------------------------------------------------- the cost prefix
def test_cost_prefix_beyond_one_chunk(eng):
    """mcq_prep_ranges_kernel is one block of 1024 threads that walks the records in chunks of 1024 and carries the sum:
    1100 records need a second chunk, and records 1024..1099 take their place on the cost axis from the carry.  A wrong
    prefix there hands their tasks to no wave or to two, and the rows differ.  Runs cycle through 1..17 (one task per
    record), 2 and 3 seats, every street."""
    tables = narrow_tables(4, 37)
    recs = [(STREETS[(i // 2) % 4], [(i + s) % 4 for s in range(2 + i % 2)], 1 + i % 17) for i in range(1100)]
    check(eng, recs, tables, 6000, alone=[0, 1023, 1024, 1099])
