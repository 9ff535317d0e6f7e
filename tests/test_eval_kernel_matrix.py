"""Every instance of the plain-query kernels against the oracle, bit for bit.

tools/isa_resched.py re-orders the vector instructions of every `mcq_eval*` kernel on its way into the library, so each
instance is its own piece of machine code and needs its own comparison with the oracle (oracle/mcq_oracle.c):
  * mcq_eval_kernel<M, SPLIT>: M = 0 production law (O.MODE_CTR), 2 uniform law (O.MODE_CTR_UNIFORM), 1 replay
    (O.MODE_MT); SPLIT = the small-batch cut of a 1024-iteration task into 2^split sub-tasks of 16 >> split iterations
    per lane (mcq_pick_split in csrc/mcq_device.hpp), false = no cut;
  * mcq_eval_direct_kernel<M>: the one-launch path of small queries (at most eight tasks), M = 0 and 2.
Run counts sit at the edges of a sub-task, a task and the cut; 1 to 10 players on every street; a seed above 2^40 so
that both key words of the counter-mode streams matter; a non-zero first query id.
"""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RUNS = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097, 16385]
SEED = (1 << 41) | 0x9E3779B97   # >= 2^40: the high key word is not zero
MT_SEED = 0x7F4A7C15             # the replay streams are MT19937, seeded with 32 bits
FQ = 1000003
LAWS = (("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM))
THREADS = 16


def u64(r):
    return r.view(np.uint64).reshape(-1, 13)


GRID = {(p, nb) for p in range(1, 11) for nb in (0, 3, 4, 5)}    # 40 (players, table cards) pairs = kernel instances


def pair(g):
    """grid cell g (mod 40): players 1 + g % 10 on street g // 10 -- unlike (1 + i % 10, i % 4), whose two coordinates
    share the parity of i and so reach only 20 of the 40 cells"""
    return 1 + g % 10, [0, 3, 4, 5][g // 10 % 4]


def batch(runs, rng, cells=None):
    """one query per run count; query i sits in grid cell cells[i] (default: i)"""
    hole, board, npl = [], [], []
    for i in range(len(runs)):
        p, nb = pair(i if cells is None else cells[i])
        c = rng.permutation(52)[:2 + nb]
        hole.append(c[:2])
        board.append(list(c[2:]) + [255] * (5 - nb))
        npl.append(p)
    q = npa.pack_queries(hole, board, npl, list(runs))
    assert_grid(q)
    return q


def assert_grid(q):
    """every batch of this file visits ALL 40 instances, each of them once with more than one task and once with a run
    count that leaves a partly filled stream (not a multiple of 16)"""
    raw = q.view(np.uint8).reshape(-1, 16)
    cells = list(zip(raw[:, 8].tolist(), raw[:, 7].tolist()))
    assert set(cells) == GRID, sorted(GRID - set(cells))
    runs = q["runs"].astype(np.int64)
    assert {c for c, r in zip(cells, runs) if r > 1024} == GRID
    assert {c for c, r in zip(cells, runs) if r % 16} == GRID


def grid_runs(extra, shift):
    """-> (runs, cells): every cell with 1025 iterations (two tasks, the second one a single iteration), then the run
    counts `extra` on cells spread over the grid (7 is coprime to 40) from `shift` on"""
    return [1025] * 40 + list(extra), list(range(40)) + [(shift + 7 * j) % 40 for j in range(len(extra))]


def tasks(q):
    return (q["runs"].astype(np.int64) + 1023) // 1024


def pick_split(q, n_cu, split_max):
    """the host's cut for a batch (mcq_pick_split): as fine as split_max allows while 2^split times the tasks stay
    within eight per CU and 512 per query.  tests/test_plan_host.py holds this mirror to the header."""
    total, most = int(tasks(q).sum()), int(tasks(q).max())
    s = 0
    while s < split_max and total << (s + 1) <= 8 * n_cu and most << (s + 1) <= 512:
        s += 1
    return s


def oracle(omode, q, seed, fq=FQ):
    return O.run_batch(omode, q.view(np.uint8).reshape(-1, 16), seed, first_qid=fq, threads=THREADS)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def device_entry(e, q, seed, fq=FQ):
    """eval_batch_device: the queries resident in HBM, the prep kernel picks the cut"""
    import torch
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    out = torch.full((len(q), 13), -7, dtype=torch.int64, device=dev)
    e.eval_batch_device(d_q.data_ptr(), len(q), seed, out.data_ptr(), first_query_id=fq)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def test_general_path_at_every_cut_under_both_laws(monkeypatch):
    """mcq_eval_kernel<0|2, false> (MCQ_SPLIT_MAX=0) and <0|2, true> at the cuts 1 to 4, host and device entries; each
    query alone too, which the finest cut reaches whatever its run count"""
    rng = np.random.default_rng(2024)
    runs, cells = grid_runs(RUNS + RUNS[:9], 3)  # 61 queries, 122 tasks: every cell, every run count of RUNS
    q = batch(runs, rng, cells)
    assert set(RUNS) <= set(runs) and int(tasks(q).sum()) == 122
    cus = n_cu()
    assert pick_split(q, cus, 4) == 4            # so MCQ_SPLIT_MAX=s really gives the cut s
    assert all(pick_split(q[i:i + 1], cus, 4) == 4 for i in range(len(q)))
    want = {law: oracle(om, q, SEED) for law, om in LAWS}
    monkeypatch.setenv("MCQ_DIRECT_MAX_TASKS", "0")
    for s in range(5):
        monkeypatch.setenv("MCQ_SPLIT_MAX", str(s))
        e = npa.Engine(0)
        try:
            for law, _ in LAWS:
                e.set_dealing_law(law)
                assert np.array_equal(u64(e.eval_batch(q, SEED, first_query_id=FQ)), want[law]), (s, law)
                assert np.array_equal(device_entry(e, q, SEED), want[law]), (s, law, "device")
                for i in range(len(q)):
                    got = u64(e.eval_batch(q[i:i + 1], SEED, first_query_id=FQ + i))
                    assert np.array_equal(got, want[law][i:i + 1]), (s, law, runs[i], pair(cells[i]))
                    got = device_entry(e, q[i:i + 1], SEED, FQ + i)
                    assert np.array_equal(got, want[law][i:i + 1]), (s, law, runs[i], pair(cells[i]), "device")
        finally:
            e.close()


def test_replay_at_every_cut(monkeypatch):
    """mcq_eval_kernel<1, false> and <1, true>: replay mode's lanes take four iterations at a time, so its cut stops at 2"""
    rng = np.random.default_rng(77)
    runs, cells = grid_runs(RUNS + RUNS[:9], 5)
    q = batch(runs, rng, cells)
    assert set(RUNS) <= set(runs)
    want = oracle(O.MODE_MT, q, MT_SEED)
    monkeypatch.setenv("MCQ_DIRECT_MAX_TASKS", "0")
    for s in range(3):
        monkeypatch.setenv("MCQ_SPLIT_MAX", str(s))
        e = npa.Engine(0)
        try:
            got = u64(e.eval_batch(q, MT_SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
            assert np.array_equal(got, want), s
            for i in range(len(q)):
                got = u64(e.eval_batch(q[i:i + 1], MT_SEED, first_query_id=FQ + i, mode=npa.MODE_REPLAY_MT19937))
                assert np.array_equal(got, want[i:i + 1]), (s, runs[i], pair(cells[i]))
        finally:
            e.close()


def test_bulk_batches_under_both_laws(monkeypatch):
    """more than 1024 queries: never cut (mcq_eval_kernel<0|2, false>), host and device entries"""
    rng = np.random.default_rng(5)
    runs = rng.choice(RUNS[:10], 1100)
    runs[::97] = 4097
    runs[1000:1040] = 1025                       # query i sits in cell i % 40: every cell once with two tasks
    q = batch(runs, rng)
    monkeypatch.setenv("MCQ_DIRECT_MAX_TASKS", "0")
    e = npa.Engine(0)
    try:
        assert pick_split(q, n_cu(), 4) == 0
        for law, om in LAWS:
            want = oracle(om, q, SEED)
            e.set_dealing_law(law)
            assert np.array_equal(u64(e.eval_batch(q, SEED, first_query_id=FQ)), want), law
            assert np.array_equal(device_entry(e, q, SEED), want), (law, "device")
    finally:
        e.close()


def test_one_launch_kernel_under_both_laws(monkeypatch):
    """mcq_eval_direct_kernel<0> and <2> under the default knobs: queries of at most eight tasks, laid out by the host
    (fewer than 128 queries) or by the kernel itself (from 128 on), and each query alone"""
    monkeypatch.delenv("MCQ_DIRECT_MAX_TASKS", raising=False)
    monkeypatch.delenv("MCQ_SPLIT_MAX", raising=False)
    rng = np.random.default_rng(31)
    short = [r for r in RUNS if r <= 8 * 1024] + [8192]
    runs, cells = grid_runs(short * 2, 11)       # 64 queries: laid out by the host
    few = batch(runs, rng, cells)
    runs_many = rng.choice(short, 200)
    runs_many[160:200] = 1025
    many = batch(runs_many, rng)
    assert set(short) <= set(runs) and len(few) < 128 <= len(many)
    assert int(tasks(few).max()) <= 8 and int(tasks(many).max()) <= 8
    e = npa.Engine(0)
    try:
        for law, om in LAWS:
            e.set_dealing_law(law)
            for q in (few, many):
                want = oracle(om, q, SEED)
                assert np.array_equal(u64(e.eval_batch(q, SEED, first_query_id=FQ)), want), (law, len(q))
            want = oracle(om, few, SEED)
            for i in range(len(few)):
                got = u64(e.eval_batch(few[i:i + 1], SEED, first_query_id=FQ + i))
                assert np.array_equal(got, want[i:i + 1]), (law, runs[i], pair(cells[i]))
    finally:
        e.close()
