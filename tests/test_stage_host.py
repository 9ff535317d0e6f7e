"""What a block of the Monte-Carlo kernels decides before its waves start, without a GPU (csrc/mcq_stage.hpp through
tests/hostsim_stage): the header is what mcq_kernels.hip compiles, so what these tests see is what a block decides from
its records.  One thing is NOT held here: which records a block of mcq_eval_ranges_kernel has.  This file takes them from
mcq_axis_block_records, while thread 0 of that kernel keeps the two prefix searches written out; that the two
agree is held on the device only, by tests/test_ranges_paths_gpu.py.

  * extended queries: the Python mirror the GPU tests' expectations use (tests/ext_grid.py: stage_lists, staging) == the
    header, verdict and offsets, on the list-placement batches, on random batches of the grid and at the edges by hand;
  * a range per seat: the shapes of tests/test_ranges_paths_gpu.py take the path their docstrings state;
  * candidate lists: the two per-thread steps, in both shapes the kernels run them, give the serial list."""
import numpy as np
import pytest

from tests import ext_grid as G
from tests import hostbuild
from tests import hostsim_ext_ways as H
from tests import hostsim_stage as S
from tests import ranges_paths as RP

N_CU = 256


# ------------------------------------------------------------------------------------------------------ extended queries
def test_limits_of_the_mirror_are_the_headers():
    c = S.consts()
    assert (G.STAGE_ENTRIES, G.STAGE_LISTS) == (c["ext_entries"], c["ext_lists"]) == (18 * 1024, 96)
    assert (c["ranges_tables"], c["ranges_queries"]) == (6, 32)


def holds(cnts, stride, qa, nq):
    """the mirror's verdict and offsets for one block are the header's; -> the verdict"""
    verdict, off = G.stage_lists(cnts, stride, qa, nq)
    staged, got = S.ext_lists(qa, nq, stride, cnts)
    assert staged == (verdict == "staged"), (verdict, qa, nq)
    assert got == [off.get(k, S.NOT_WRITTEN) for k in range(len(got))], (verdict, qa, nq, stride)
    return verdict


def batch_holds(recs, n_cu, occ):
    stride = max(max(r.lists for r in recs), 1)
    cnts = G.list_counts(recs, stride)
    blocks = G.staging(recs, n_cu, occ, offsets=True)
    for verdict, qa, nq, off in blocks:
        assert holds(cnts, stride, qa, nq) == verdict and G.stage_lists(cnts, stride, qa, nq)[1] == off
    return {v for v, _, _, _ in blocks}


@pytest.mark.parametrize("name,want", [("staged", {"staged"}), ("no_block_stages", {"entries"}),
                                       ("refused_by_entries", {"entries"}), ("refusing_beside_staging", {"entries", "staged"})])
def test_placement_batches_mirror_is_the_header(name, want):
    recs, _ = G.placement_batches()[name]
    for occ in (1, 2):
        assert batch_holds(recs, N_CU, occ) == want, (name, occ)


def test_random_batches_of_the_grid_mirror_is_the_header():
    """Seeded batches drawn from the grid, 1 to 400 records, on 1 to 256 compute units at both occupancies: few units give
    blocks of many records, where the count refuses and the entries run over in the middle of a block."""
    rng = np.random.default_rng(G.GEN_SEED + 7)
    grid, seen = G.grid(), set()
    for _ in range(40):
        recs = [grid[i] for i in rng.integers(0, len(grid), int(rng.integers(1, 401)))]
        seen |= batch_holds(recs, int(rng.choice([1, 2, 3, 8, 64, 256])), int(rng.integers(1, 3)))
    assert seen == {"staged", "count", "entries"}


def test_staging_edges_by_hand():
    cap = G.STAGE_ENTRIES
    # exactly 96 lists, and 97: the closing offset of 96 lists is the array's last entry
    assert holds([10] * 99, 1, 3, 96) == "staged" and S.ext_lists(3, 96, 1, [10] * 99)[1][96] == 960
    assert holds([10] * 100, 1, 3, 97) == "count" and set(S.ext_lists(3, 97, 1, [10] * 100)[1]) == {S.NOT_WRITTEN}
    assert holds([5] * 96, 6, 0, 16) == "staged" and holds([5] * 102, 6, 0, 17) == "count"
    assert holds([5] * 100, 10, 1, 9) == "staged" and holds([5] * 100, 10, 0, 10) == "count"
    # offsets that land exactly on the capacity, and one word beyond
    assert holds([cap // 2, cap // 2], 1, 0, 2) == "staged" and S.ext_lists(0, 2, 1, [cap // 2, cap // 2])[1][:3] == [0, cap // 2, cap]
    assert holds([cap // 2, cap // 2 + 1], 1, 0, 2) == "entries" and S.ext_lists(0, 2, 1, [cap // 2, cap // 2 + 1])[1][2] == cap + 2
    assert holds([cap - 2, 1], 1, 0, 2) == "staged" and holds([cap - 2, 2, 1], 1, 0, 3) == "entries"
    # an odd length takes a whole word more: the next list begins on an even entry
    assert holds([7, 1, 0, 3], 4, 0, 1) == "staged" and S.ext_lists(0, 1, 4, [7, 1, 0, 3])[1][:5] == [0, 8, 10, 10, 14]
    assert holds([cap - 1], 1, 0, 1) == "staged" and holds([cap - 1, 1], 1, 0, 2) == "entries"
    # overflow at the first list (nothing behind it is looked at: its offset and the closing one) and at the last
    staged, off = S.ext_lists(0, 3, 1, [cap + 1, 4, 4])
    assert not staged and off[:4] == [0, S.NOT_WRITTEN, S.NOT_WRITTEN, cap + 2] and holds([cap + 1, 4, 4], 1, 0, 3) == "entries"
    staged, off = S.ext_lists(1, 3, 1, [9999, 4, 4, cap])
    assert not staged and off[:4] == [0, 4, 8, cap + 8] and holds([9999, 4, 4, cap], 1, 1, 3) == "entries"
    # a block without a piece of the axis
    assert S.ext_lists(0, 0, 3, [1, 2, 3]) == (False, [S.NOT_WRITTEN] * 97)


# ------------------------------------------------------------------------------------------------------ a range per seat
def drawn_tables(recs, tables, first, count):
    """The distinct tables the records' seats draw from, in the order they name them: a table with one entry is a known
    hand and draws nothing."""
    out = []
    for _, st, _ in recs[first:first + count]:
        for t in st:
            if np.count_nonzero(tables[t]) != 1 and t not in out:
                out.append(t)
    return out


def check_slots(recs, tables, first, count, staged):
    """the look-up at a record's start finds the slot of every table the record draws from"""
    for t in drawn_tables(recs, tables, first, count):
        assert staged[S.ranges_slot(staged, t)] == t


@pytest.mark.parametrize("shape", RP.THRESHOLD_SHAPES)
def test_threshold_shapes_take_the_stated_path(shape):
    """What test_ranges_paths_gpu.test_staging_thresholds_in_one_block states of each shape, from the kernel's own rule:
    with MCQ_GRID_CAP=1 one block holds every record of the call."""
    recs, tables = RP.threshold_shape(shape)
    q, seat_table = RP.batch(recs)
    _, blocks = S.ranges_blocks(q, seat_table, tables, N_CU, grid_cap=1)
    assert len(blocks) == 1
    first, count, staged = blocks[0]
    assert (first, count) == (0, len(recs))
    drawn = drawn_tables(recs, tables, 0, count)
    if shape == "32 records, 6 tables":
        assert count == 32 and sorted(staged) == list(range(6)) and staged == drawn       # all six slots in use
    elif shape == "32 records, 7 tables":
        assert count == 32 and len(drawn) == 7 and staged == []                           # the seventh table refuses
    elif shape == "33 records, 6 tables":
        assert count == 33 and len(drawn) == 6 and staged == []                           # the 33rd record refuses
    elif shape == "32 records, 6 tables and 4 known hands":
        named = {t for _, st, _ in recs for t in st}
        assert count == 32 and len(named) == 10 and sorted(named - set(drawn)) == [6, 7, 8, 9]   # ten named, four known hands
        assert sorted(staged) == list(range(6)) and staged == drawn
    else:
        assert shape == "known hands only" and drawn == [] and staged == []                # nothing to stage
    if staged:
        check_slots(recs, tables, 0, count, staged)


def test_mixed_batch_blocks_stage_refuse_and_straddle():
    """test_ranges_paths_gpu.test_blocks_that_stage_beside_blocks_that_do_not on 256 compute units: 144 blocks of four
    waves; which of them stage, which refuse on tables, and where the two halves of the batch meet."""
    recs, tables = RP.mixed_batch()
    q, seat_table = RP.batch(recs)
    prefix, blocks = S.ranges_blocks(q, seat_table, tables, N_CU)
    assert len(blocks) == 144 and all(0 < count <= 3 for _, count, _ in blocks)
    assert all(prefix[i] < prefix[i + 1] for i in range(48))
    staging, refusing, straddling = [], [], []
    for b, (first, count, staged) in enumerate(blocks):
        drawn = drawn_tables(recs, tables, first, count)
        assert staged == (drawn if len(drawn) <= 6 else []), b
        if staged:
            staging.append(b)
            check_slots(recs, tables, first, count, staged)
        else:
            refusing.append(b)                       # (no block of this batch has more than 32 records or known hands only)
            if first < 24 <= first + count - 1:
                straddling.append(b)
    assert staging and refusing and straddling
    # the block numbers the GPU test's docstring gives
    assert staging == list(range(0, 68)) and straddling == [68] and refusing == list(range(68, 144))
    assert any(len(blocks[b][2]) < 6 for b in staging) and all(blocks[b][0] >= 24 for b in refusing[1:])
    assert blocks[68][:2] == (23, 2) and len(drawn_tables(recs, tables, 23, 2)) == 15    # five tables of record 23, ten of record 24


# ------------------------------------------------------------------------------------------------------ candidate lists
def in_order(lst):
    """entries a | b << 8 in the strictly ascending order of 52 * a + b"""
    c = 52 * (lst & 0xFF).astype(np.int64) + (lst >> 8)
    return bool((np.diff(c) > 0).all()) and (len(c) == 0 or (0 <= c[0] and c[-1] < 2704))


def test_compaction_gives_the_serial_list_for_every_record_of_the_grid():
    """The serial list comes from the same two functions, one candidate per thread (tests/hostsim/hs_walk.hpp).  What does
    not share their code: the order check here, hostsim_ext_ways.list_len, the list built in Python in
    test_compaction_edges and the sanitizer program's own loop."""
    seen, lists = set(), 0
    for r in G.grid():
        if r.key in seen:
            continue
        seen.add(r.key)
        for li in range(r.lists):
            serial = S.serial_list(r.q, r.ext, li)
            U, cls = S.list_plan(r.q, r.ext, li)
            assert len(serial) == H.list_len(r.q, r.ext, li) and in_order(serial), (r, li)
            for per in S.THREADS:
                assert np.array_equal(S.compact(per, U, cls), serial), (r, li, per)
            lists += 1
    assert lists > 300


EVERY = np.array([0xFFFFFFFF] * 5 + [0x1FF], np.uint32)


def test_compaction_edges():
    full = (1 << 52) - 1
    want = np.array([a | b << 8 for a in range(52) for b in range(52) if a != b], np.uint16)
    for per, threads in S.THREADS.items():
        assert len(S.compact(per, full, np.zeros(6, np.uint32))) == 0 and len(S.compact(per, 0, EVERY)) == 0   # empty
        # the full deck, every class: 2652 entries; the thread that holds candidate 2703 also holds candidates past the end
        masks = S.list_masks(per, full, EVERY)
        straddle = 2703 // per
        assert straddle * per <= 2703 < 2704 < (straddle + 1) * per and straddle < threads
        assert int(masks[straddle]) == (1 << (2703 - straddle * per)) - 1 and not masks[straddle + 1:].any()   # 2703 is (51, 51): no hand
        assert np.array_equal(S.compact(per, full, EVERY), want) and len(want) == 2652
        # survivors in the last thread that holds any only: it writes from offset 0, nobody else writes
        last = 2702 // per
        only = np.zeros(threads, np.uint32)
        only[last] = masks[last]
        n = bin(int(masks[last])).count("1")
        got = S.list_scatter(per, only, np.zeros(threads, np.uint32), n)
        assert n >= 2 and np.array_equal(got, want[-n:])
        # ... and behind a full first thread
        only[0] = masks[0]
        first_n = bin(int(masks[0])).count("1")
        at = np.zeros(threads, np.uint32)
        at[1:] = first_n
        assert np.array_equal(S.list_scatter(per, only, at, first_n + n), np.concatenate([want[:first_n], want[-n:]]))


def test_sanitized_program(tmp_path):
    """Every function at the bounds of its arrays -- 96 lists and their 97th offset, six tables and a seventh, 32 and 33
    records, list strides 1 and 10, both compactions -- under AddressSanitizer and UndefinedBehaviorSanitizer."""
    lines = hostbuild.run_sanitized("hostsim_stage/hs_main.cpp", "-O1", tmp_path)
    assert lines[-1] == "ok: 19" and all(ln.endswith(": holds") for ln in lines[:-1]), lines
