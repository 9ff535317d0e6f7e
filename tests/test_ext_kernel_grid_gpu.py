"""Every form of the extended-query kernels against the host build of the lane code, bit for bit, over the grid of
tests/ext_grid.py (whose expected rows tests/test_ext_kernel_grid_host.py pins to the oracle).

  * mcq_eval_ext_kernel<MODE_PHILOX, ROW>, ROW = hero row (mcq_eval_batch_ext), MCQ_ROW_WAYS (.._ext_ways), MCQ_ROW_SEATS
    (.._ext_seats): mcq_iteration_ext_fast and mcq_iteration_ext, the candidate lists staged in LDS or read from HBM,
    streams of 2 and of 16 iterations side by side on one wave's slice of the cost axis;
  * mcq_eval_ext_small_kernel<WAYS>, the one-launch path, at 4, 8 and 16 working waves per block, one to sixteen parts
    per query, exactly 32 blocks, streams of 2 and of 16;
  * the fences between the two (6 / 7 lists, 64 / 65 tasks, 8 / 9 queries).
Which path, which cut and which list placement a batch gets is not observable from outside: the choices of
eval_batch_ext_impl (through csrc/mcq_plan.hpp) and of the kernel's staging step are mirrored in tests/ext_grid.py
(held to the headers on the host by tests/test_plan_host.py and tests/test_axis_host.py) and the intended value is
asserted for every batch."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from tests import ext_grid as G
from tests import ext_ways_cases as XC
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB


def engine(monkeypatch, small):
    """small=False: MCQ_EXT_SMALL=0, nothing escapes to the one-launch kernel; True: the default knobs."""
    if small:
        monkeypatch.delenv("MCQ_EXT_SMALL", raising=False)
    else:
        monkeypatch.setenv("MCQ_EXT_SMALL", "0")
    return npa.Engine(0)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def words(rows, n):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, n)


def check(e, recs, fq, seats=True, what=None):
    """All row kinds of one call against the host rows -> the 22-word rows."""
    q, ext = G.pack(recs)
    exp_ways, exp_seats = G.expect(recs, fq, seats=seats)
    ways = words(e.eval_batch_ext_ways(q, ext, G.SEED, first_query_id=fq), 22)
    bad = np.flatnonzero((ways != exp_ways).any(1))
    assert not len(bad), (what, "ways", [(int(j), recs[j]) for j in bad[:5]])
    hero = np.ascontiguousarray(e.eval_batch_ext(q, ext, G.SEED, first_query_id=fq))
    assert ways[:, :13].tobytes() == hero.tobytes(), (what, "hero rows")
    if seats:
        got = words(e.eval_batch_ext_seats(q, ext, G.SEED, first_query_id=fq), 32)
        bad = np.flatnonzero((got != exp_seats).any(1))
        assert not len(bad), (what, "seats", [(int(j), recs[j]) for j in bad[:5]])
        assert np.array_equal(got[:, :4], ways[:, :4]), (what, "seats against ways")
        assert [int(x) for x in got[:, 4]] == [SE.hero_share_from_ways(w) for w in ways], (what, "hero's share")
    return ways


# ---- the general path over the grid
def test_general_path_whole_grid(monkeypatch):
    """mcq_eval_ext_kernel<PHILOX, hero | WAYS | SEATS>: every cell of the grid in one launch, fast and general form,
    lists staged (a block holds few queries), streams of 2 and of 16 iterations on the same waves."""
    e = engine(monkeypatch, False)
    try:
        recs = G.grid()
        G.assert_grid(recs)
        check(e, recs, G.FQ)
    finally:
        e.close()


def test_general_path_shuffled_grid(monkeypatch):
    e = engine(monkeypatch, False)
    try:
        recs, fq = G.shuffled()
        rules = [(r.s_iters, bool(r.lists)) for r in recs]
        # the three kinds of neighbours the stream rule makes: list-less on 16, listed on 2, listed on 16
        trios = {frozenset(rules[j:j + 3]) for j in range(len(rules) - 2)}
        assert frozenset({(16, False), (2, True), (16, True)}) in trios
        check(e, recs, fq)
    finally:
        e.close()


def test_general_path_every_record_alone(monkeypatch):
    """One query per launch: its tasks spread over one-task blocks, whatever its run count."""
    e = engine(monkeypatch, False)
    try:
        for j, r in enumerate(G.grid()):
            check(e, [r], G.FQ + j, what=j)
    finally:
        e.close()


# ---- the one-launch path
@pytest.mark.parametrize("name", list(G.small_batches()))
def test_one_launch_path(monkeypatch, name):
    """mcq_eval_ext_small_kernel<false | true> under the default knobs, the cut the host must choose asserted, against the
    host rows and against the same batch on the general path."""
    recs, fq, want = G.small_batches()[name]
    plan = G.small_plan(recs)
    assert plan is not None and (plan[0], plan[2]) == want
    e = engine(monkeypatch, True)
    try:
        ways = check(e, recs, fq, seats=False, what=name)
    finally:
        e.close()
    e = engine(monkeypatch, False)
    try:
        assert np.array_equal(check(e, recs, fq, seats=False, what=(name, "general")), ways)
    finally:
        e.close()


@pytest.mark.parametrize("name", list(G.fence_batches()))
def test_fences_between_the_paths(monkeypatch, name):
    """6 lists, 64 tasks and 8 queries take one launch; 7 or 10 lists, 65 tasks and 9 queries take the general path; the
    rows are the host's on either side, and equal with the one-launch kernel switched off."""
    recs, fq, small = G.fence_batches()[name]
    assert (G.small_plan(recs) is not None) == small
    e = engine(monkeypatch, True)
    try:
        ways = check(e, recs, fq, what=name)
    finally:
        e.close()
    e = engine(monkeypatch, False)
    try:
        assert np.array_equal(check(e, recs, fq, seats=False, what=(name, "general")), ways)
    finally:
        e.close()


# ---- where the candidate lists are read from
def assert_verdicts(recs, want):
    verdicts, blocks = G.placement_verdicts(recs, n_cu())
    assert verdicts == [want] * 2, verdicts     # at one and at two resident blocks per CU
    return blocks


@pytest.mark.parametrize("name,want", [("staged", {"staged"}), ("no_block_stages", {"entries"}),
                                       ("refused_by_entries", {"entries"}),
                                       ("refusing_beside_staging", {"entries", "staged"})])
def test_list_placement(monkeypatch, name, want):
    """(a) every block stages; (b) no block can: every query alone overflows the LDS buffer, seats rows included --
    mcq_iteration_ext<.., false, McqLaneAccSeats>; (c) the fast form from HBM, staging refused by the entries, not by the
    number of lists; (d) refusing and staging blocks in one launch."""
    recs, fq = G.placement_batches()[name]
    assert G.small_plan(recs) is None
    blocks = assert_verdicts(recs, want)
    if name == "refused_by_entries":
        assert all(nq <= G.STAGE_LISTS for b in blocks for _, _, nq in b)      # one list per query: never by count
    if name == "refusing_beside_staging":
        for b in blocks:     # the fat third lies in refusing blocks, and some thin queries in staging blocks only
            assert all(v == "entries" for v, qa, nq in b if qa < len(recs) // 3)
            assert any(v == "staged" and qa >= len(recs) // 3 for v, qa, nq in b)
    e = engine(monkeypatch, True)
    try:
        check(e, recs, fq, what=name)
    finally:
        e.close()


def test_list_placement_refused_by_count_seats_rows(monkeypatch):
    """(e) the construction of test_ext_ways_gpu.test_general_path_staging_refused -- one record with ten lists among six
    thousand: every block holds more than 96 lists -- for all three row kinds."""
    wide = dict(name="wide", hero=set(XC.top_classes(0.5)), board=[], n=10, opp=XC.top_classes(0.5),
                known=[set(XC.top_classes(0.5))] * 8)
    distinct = [G.Rec("wide", *XC.records(wide, 64))] + [G.Rec("case", *XC.records(XC.CASES[i], 64)) for i in (5, 0)]
    recs = [distinct[0]] + [distinct[1 + (j & 1)] for j in range(1, 6000)]
    assert_verdicts(recs, {"count"})
    e = engine(monkeypatch, True)
    try:
        check(e, recs, G.FQ + 60000, what="refused by count")
    finally:
        e.close()


# ---- errors in the middle of a batch
def raw(e, entry, q, ext, fq, n_words):
    out = np.full(len(q) * n_words, SENTINEL, np.uint64)
    rc = getattr(e._lib, entry)(e._ctx, q.ctypes.data, ext.ctypes.data, len(q), G.SEED, fq, npa.MODE_PHILOX, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("small", [True, False], ids=["one_launch", "general"])
@pytest.mark.parametrize("fault", ["undealable", "invalid"])
def test_error_in_the_middle_of_a_batch(monkeypatch, small, fault):
    """An undealable record / an invalid one between grid records: MCQ_EINVAL, and `out` untouched, for every row kind."""
    recs = G.fence_batches()["eight_queries" if small else "nine_queries"][0][:7 if small else 9]
    q, ext = G.pack(recs)
    q, ext = q.copy(), ext.copy()
    mid = len(recs) // 2
    if fault == "undealable":
        q[mid], ext[mid] = [x[0] for x in XC.records(XC.UNDEALABLE, 64)]
    else:
        q["hole"][mid] = q["hole"][mid][0]    # a card named twice
        ext["hero_is_range"][mid] = 0
    e = engine(monkeypatch, True)
    try:
        for entry, n_words in (("mcq_eval_batch_ext", 13), ("mcq_eval_batch_ext_ways", 22), ("mcq_eval_batch_ext_seats", 32)):
            rc, out = raw(e, entry, q, ext, G.FQ, n_words)
            assert rc == _lib.MCQ_EINVAL and (out == SENTINEL).all(), (entry, rc)
        good_q, good_ext = G.pack(recs)      # the same call without the fault goes through
        rc, out = raw(e, "mcq_eval_batch_ext_ways", good_q, good_ext, G.FQ, 22)
        assert rc == 0 and (out != SENTINEL).any()
    finally:
        e.close()
