"""Hot boards (tests/hot_boards.py: situations in which straight flushes, quads, full houses and ties are common)
through every Monte-Carlo kernel, bit for bit against the oracle: mcq_eval_kernel with and without the sub-task cut,
mcq_eval_direct_kernel, replay, the device entries, the split-pot entries and the extended kernels (a record that
restricts nothing, and one ranged opponent class set).  Both dealing laws where the entry has them."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import hot_boards as B
from tests import ways_expect as W

pytestmark = pytest.mark.gpu
LAWS = (("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM))


def u64(r, w=13):
    return np.ascontiguousarray(r).view(np.uint64).reshape(-1, w)


def q16():
    return B.queries().view(npa.QUERY_DTYPE).reshape(-1)


def on_device(fn, q, seed, fq, width=13):
    import torch
    d_q = torch.from_numpy(q.view(np.uint8).reshape(-1, 16).copy()).cuda()
    out = torch.full((len(q), width), -7, dtype=torch.int64, device="cuda")
    fn(d_q.data_ptr(), len(q), seed, out.data_ptr(), first_query_id=fq)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("knobs", [{"MCQ_DIRECT_MAX_TASKS": "0", "MCQ_SPLIT_MAX": "0"}, {"MCQ_DIRECT_MAX_TASKS": "0"}, {}],
                         ids=["uncut", "cut", "one-launch"])
def test_plain_kernels_on_the_list(monkeypatch, knobs):
    for k in ("MCQ_DIRECT_MAX_TASKS", "MCQ_SPLIT_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    q = q16()
    e = npa.Engine(0)
    try:
        for law, om in LAWS:
            want = B.expected(om)
            e.set_dealing_law(law)
            assert np.array_equal(u64(e.eval_batch(q, B.SEED, first_query_id=B.QID)), want), law
            assert np.array_equal(on_device(e.eval_batch_device, q, B.SEED, B.QID), want), (law, "device")
            assert np.array_equal(on_device(e.eval_batch_device_small, q, B.SEED, B.QID), want), (law, "device small")
            for i in range(len(q)):
                got = u64(e.eval_batch(q[i:i + 1], B.SEED, first_query_id=B.QID + i))
                assert np.array_equal(got, want[i:i + 1]), (law, B.cases()[i])
        e.set_dealing_law("reference")
        want = B.expected(O.MODE_MT)
        got = u64(e.eval_batch(q, B.MT_SEED, first_query_id=B.QID, mode=npa.MODE_REPLAY_MT19937))
        assert np.array_equal(got, want), "replay"
    finally:
        e.close()


def test_split_pot_entries_on_the_list():
    q = q16()
    e = npa.Engine(0)
    try:
        for omode, mode, law, seed in ((O.MODE_CTR, npa.MODE_PHILOX, "reference", B.SEED),
                                       (O.MODE_CTR_UNIFORM, npa.MODE_PHILOX, "uniform", B.SEED),
                                       (O.MODE_MT, npa.MODE_REPLAY_MT19937, "reference", B.MT_SEED)):
            e.set_dealing_law(law)
            want = np.stack([W.expected_row(omode, h, t, n, B.RUNS, seed, B.QID + i) for i, (h, t, n) in enumerate(B.cases())])
            assert np.array_equal(want[:, :13], B.expected(omode))
            got = u64(e.eval_batch_ways(q, seed, first_query_id=B.QID, mode=mode), 22)
            assert np.array_equal(got, want), (law, mode)
            if mode == npa.MODE_PHILOX:
                assert np.array_equal(on_device(e.eval_batch_device_ways, q, seed, B.QID, 22), want), (law, "device")
    finally:
        e.close()


def test_extended_kernels_on_the_list():
    q = q16()
    e = npa.Engine(0)
    try:
        plain = B.expected(O.MODE_CTR)
        free = npa.pack_query_ext(len(q))
        assert np.array_equal(u64(e.eval_batch_ext(q, free, B.SEED, first_query_id=B.QID)), plain)       # the general path
        for lo in range(0, len(q), 8):                                                                   # at most eight: one launch
            got = u64(e.eval_batch_ext(q[lo:lo + 8], free[lo:lo + 8], B.SEED, first_query_id=B.QID + lo))
            assert np.array_equal(got, plain[lo:lo + 8]), lo
        idx = [i for i, (_, _, n) in enumerate(B.cases()) if n > 1]
        ranged = npa.pack_query_ext(len(q), opp_range=npa.range_bits(B.RANGE))
        whole = u64(e.eval_batch_ext(q, ranged, B.SEED, first_query_id=B.QID))
        for i in idx:
            hero, table, n = B.cases()[i]
            want = O.run_ex(O.MODE_CTR, hero, table, n, B.RUNS, B.SEED, qid=B.QID + i, opp_range=B.RANGE)["tallies"]
            assert np.array_equal(whole[i], want), (hero, table, n)
            got = u64(e.eval_batch_ext(q[i:i + 1], ranged[i:i + 1], B.SEED, first_query_id=B.QID + i))
            assert np.array_equal(got[0], want), (hero, table, n, "one launch")
    finally:
        e.close()
