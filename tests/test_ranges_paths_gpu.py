"""The parts of mcq_eval_batch_ranges that exist only in mcq_kernels.hip -- the parallel table scan, the decision what a
block stages in LDS, the chunked cost prefix -- bit for bit against the host build of the lane code (tests/hostsim_ranges,
which prepares its tables with the serial mcq_ranges_prefix and knows neither blocks nor staging).  Which path ran cannot
be observed from outside: every docstring states, from the kernel's rule, which path its shape takes.  A sample of every
batch is sent again record by record at the matching first_query_id, where a record is alone in its block."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from tests import hostsim_ranges as H
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
SEED = 20261021
BOARD = [10, 17, 34, 3, 21]   # 4H 6D TH 2S 7D: clear of every hand the scan tables name
STREETS = (3, 0, 4, 5)
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


def batch(recs):
    """recs: [(table cards, seats' table numbers, runs)] -> (queries, seat_table [n, 10])"""
    q = np.concatenate([_lib.pack_query_one([0, 0], BOARD[:nb], len(st), runs) for nb, st, runs in recs])
    seat_table = np.full((len(recs), 10), 0xFFFFFFFF, np.uint32)   # entries at or above n_players are not read
    for i, (_, st, _) in enumerate(recs):
        seat_table[i, :len(st)] = st
    return q, seat_table


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


def narrow_tables(n, seed):
    """n distinct tables of about 300 hands, weights 1..9."""
    g = np.random.default_rng(seed)
    t = np.zeros((n, 1326), np.uint16)
    for k in range(n):
        on = g.random(1326) < 0.23
        t[k, on] = g.integers(1, 10, int(on.sum()))
    assert len({x.tobytes() for x in t}) == n
    return t


def one_hot_tables(hands):
    t = np.zeros((len(hands), 1326), np.uint16)
    for k, (a, b) in enumerate(hands):
        assert a not in BOARD and b not in BOARD
        t[k, _lib.hand_index(a, b)] = 1 + 7 * k
    return t


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
ONE_HOT = [(0, 1), (4, 5), (8, 9), (12, 13), (16, 18), (20, 22), (24, 25), (28, 29), (32, 33), (36, 37)]


def threshold_records(n, n_tables, known=False):
    """n records of 2 to 6 seats over every street, runs 1 .. 200, seat s of record i on table (i + s) % n_tables; with
    `known`, one seat of every record (two of every third) holds one of the four known hands behind the tables."""
    recs = []
    for i in range(n):
        p = 2 + i % 5
        st = [(i + s) % n_tables for s in range(p)]
        if known:
            st[i % p] = n_tables + i % 4
            if i % 3 == 0:
                st[(i + 1) % p] = n_tables + (i + 1) % 4
        recs.append((STREETS[i % 4], st, (1, 17, 64, 200, 130)[i % 5]))
    return recs


@pytest.mark.parametrize("shape", ["32 records, 6 tables", "32 records, 7 tables", "33 records, 6 tables",
                                   "32 records, 6 tables and 4 known hands", "known hands only"])
def test_staging_thresholds_in_one_block(eng_one_block, shape):
    """One block sees every record of the call.  It stages when its records are at most MCQ_RG_STAGE_QUERIES = 32 and
    name at most MCQ_RG_STAGE_TABLES = 6 distinct tables, tables with one entry not counted:
      32 records, 6 tables                     -> staged, all six slots of s_cum in use;
      32 records, 7 tables                     -> the seventh table does not fit: every draw reads HBM;
      33 records, 6 tables                     -> one record too many: HBM;
      32 records, 6 tables and 4 known hands   -> ten distinct tables, four of them known hands: staged;
      known hands only                         -> no table to stage, no draw at all: passes == runs."""
    if shape == "known hands only":
        tables = one_hot_tables(ONE_HOT)
        recs = [(STREETS[i % 4], [(i + 3 * s) % 10 for s in range(2 + i % 3)], (1, 17, 64, 200)[i % 4]) for i in range(32)]
        for _, st, _ in recs:
            assert len(set(st)) == len(st)
    else:
        n, nt = (33 if shape.startswith("33") else 32), (7 if "7 tables" in shape else 6)
        known = "known" in shape
        tables = narrow_tables(nt, 23)
        if known:
            tables = np.concatenate([tables, one_hot_tables(ONE_HOT[:4])])
        recs = threshold_records(n, nt, known)
        named = {t for _, st, _ in recs for t in st}
        assert named == set(range(len(tables)))
    got = check(eng_one_block, recs, tables, 4000, alone=[0, 5, len(recs) - 1])
    if shape == "known hands only":
        assert all(int(r[0]) == int(r[1]) for r in got)


# ------------------------------------------------------------------------------------------------------- mixed blocks
def full_width_tables():
    """Ten distinct tables with all 1326 entries non-zero (weights 1..7), each with most of its weight on the six pairs of
    one rank that is not on the flop: ten seats then collide seldom, and the host build of the reference stays cheap."""
    g = np.random.default_rng(29)
    t = g.integers(1, 8, (10, 1326)).astype(np.uint16)
    ranks = [r for r in range(13) if r not in {c >> 2 for c in BOARD[:3]}]
    for k in range(10):
        for a in range(4):
            for b in range(a + 1, 4):
                t[k, _lib.hand_index(4 * ranks[k] + a, 4 * ranks[k] + b)] = 60000
    assert (t != 0).all()
    return t


def test_blocks_that_stage_beside_blocks_that_do_not(eng):
    """48 flop records of 2500 runs (three wave tasks each) on the default grid: 144 tasks, one block of four waves per
    task.  Records 0..23 (2 to 6 seats) name tables 0..5 only, records 24..47 seat ten players on ten distinct full-width
    tables each.  A block whose piece of the cost axis lies inside the first 24 records finds at most six tables and
    stages them; one inside the last 24 finds ten and reads HBM; the block whose piece holds the end of record 23 and the
    start of record 24 finds sixteen, and its waves run BOTH kinds of record from HBM.  The cost axis is cut by price
    (seats, street, estimated trials), not by record: with the host's prices for these tables blocks 0..67 lie among the
    first 24 records (one to three records each, so fewer than six tables are staged in most), block 68 holds the change
    and blocks 69..143 lie among the last 24."""
    tables = np.concatenate([narrow_tables(6, 31), full_width_tables()])
    recs = [(3, [(i + s) % 6 for s in range(2 + i % 5)], 2500) for i in range(24)]
    recs += [(3, [6 + (i + s) % 10 for s in range(10)], 2500) for i in range(24)]
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
