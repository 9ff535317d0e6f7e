"""The opponents' cards read by the table's flush suit on the device: the straight forms of mcq_iteration_sum keep the
positions of the opponents' cards while they deal and read each card once, behind the table, from the wave's hole table
(McqDeckBySuit in mcq_eval_kernel), by the one suit that can still make a flush.  The host build of the same text:
tests/test_hole_by_suit_host.py.

Which kernels run those forms: mcq_eval_kernel in production mode, both laws, cut and uncut, plain and split-pot rows (1 to 9
opponents), and its parity instances with plain rows for 1 to 5 opponents.  The one-launch kernel (mcq_eval_direct_kernel) and
parity mode with six or more opponents run the general form, which reads the cards where they are dealt: their cases here
are regression checks of object code this does not alter.

One query per cell of 2 to 10 players x 0, 3, 4, 5 table cards (tests/bysuit_cases.py: a flop of three cards of every suit in
turn, a rainbow flop, turns split 2 + 2, four-flush turns, rivers with three, four, five and at most two of a suit; heroes
with zero, one and two cards of the table's suit), 1041 runs each: one full task of 1024 iterations and a ragged one of 17.

* uncut bulk kernel, cut bulk kernel, one-launch kernel, each through the host entry and the device-pointer entry, under both
  dealing laws: == the oracle's CTR / CTR-uniform rows bit for bit;
* split-pot rows on the same paths: the plain words == the oracle's, tie_ways == the host build of the lane code;
* parity mode, plain rows, 1 to 5 opponents (and 6, the general form) == the oracle's MT19937 walk bit for bit.
"""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import bysuit_cases
from tests import hostsim_epochs

pytestmark = pytest.mark.gpu

SEED, FQ = (1 << 46) | 0xB5017, 43
RUNS = 1041
LAWS = [("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM)]
CELLS = bysuit_cases.cells()
PATHS = {"uncut": {"MCQ_DIRECT_MAX_TASKS": "0", "MCQ_SPLIT_MAX": "0"}, "cut": {"MCQ_DIRECT_MAX_TASKS": "0"}, "one-launch": {}}


def queries(cells=CELLS, runs=RUNS):
    return bysuit_cases.pack(cells, runs, npa.pack_queries)


def raw16(q):
    return np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)


def u64(r, words=13):
    return np.ascontiguousarray(r).view(np.uint64).reshape(-1, words)


def host_ways(uniform):
    """the 22-word rows from the host build, each query through the form the kernels' dispatch gives it"""
    out = []
    for i, r in enumerate(raw16(queries())):
        nopp, ndeal = int(r[8]) - 1, 5 - int(r[7])
        ndeal = ndeal if ndeal in (5, 2, 1) and nopp <= 7 else -1
        out.append(hostsim_epochs.rows(r, SEED, FQ + i, nopp, ndeal, uniform=uniform, ways=True)[0])
    return np.stack(out)


@pytest.fixture(scope="module")
def want():
    """per law: the oracle's rows and the host build's split-pot rows -- computed once, read-only"""
    out = {}
    for law, omode in LAWS:
        w = {"plain": O.run_batch(omode, raw16(queries()), SEED, first_qid=FQ, threads=16), "ways": host_ways(law == "uniform")}
        for v in w.values():
            v.setflags(write=False)
        out[law] = w
    return out


def on_device(fn, q, width):
    import torch
    dq = torch.from_numpy(raw16(q).copy()).cuda()
    out = torch.full((len(q), width), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn(dq.data_ptr(), len(q), SEED, out.data_ptr(), first_query_id=FQ, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def test_cells_are_what_they_claim(want):
    bysuit_cases.check_coverage(CELLS)
    q = raw16(queries())
    assert RUNS == 1024 + 17 and all(int(r[12:16].view("<u4")[0]) == RUNS for r in q)
    for law, _ in LAWS:
        assert np.array_equal(want[law]["ways"][:, :13], want[law]["plain"])     # the host build itself against the oracle
        assert want[law]["ways"][:, 14:].any()                                   # pots shared three ways and more occur
        assert want[law]["plain"][:, 4 + 5].sum() > 0                            # hero wins with flushes


@pytest.mark.parametrize("path", list(PATHS))
def test_every_path_equals_the_oracle(monkeypatch, want, path):
    for k in ("MCQ_DIRECT_MAX_TASKS", "MCQ_SPLIT_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    q = queries()
    e = npa.Engine(0)
    try:
        for law, _ in LAWS:
            e.set_dealing_law(law)
            plain, ways = want[law]["plain"], want[law]["ways"]
            got = u64(e.eval_batch(q, SEED, first_query_id=FQ))
            bad = np.flatnonzero((got != plain).any(1))
            assert len(bad) == 0, (law, bad[:8], got[bad[:2]], plain[bad[:2]])
            assert np.array_equal(on_device(e.eval_batch_device, q, 13), plain), (law, "device")
            if path == "one-launch":
                assert np.array_equal(on_device(e.eval_batch_device_small, q, 13), plain), (law, "device small")
            rows = u64(e.eval_batch_ways(q, SEED, first_query_id=FQ), 22)
            bad = np.flatnonzero((rows != ways).any(1))
            assert len(bad) == 0, (law, "ways", bad[:8], rows[bad[:2]], ways[bad[:2]])
            assert np.array_equal(on_device(e.eval_batch_device_ways, q, 22), ways), (law, "device ways")
            for i in (1, 5, 18, 35):                                             # one query alone in its call
                assert np.array_equal(u64(e.eval_batch(q[i:i + 1], SEED, first_query_id=FQ + i))[0], plain[i]), (law, i)
    finally:
        e.set_dealing_law("reference")
        e.close()


def test_parity_mode_equals_the_mt_walk():
    cells = [c for c in CELLS if c[2] <= 7]          # 1 to 5 opponents: the straight parity forms; 6: the general form
    q = queries(cells)
    exp = O.run_batch(O.MODE_MT, raw16(q), SEED, first_qid=FQ, threads=16)
    e = npa.Engine(0)
    try:
        got = u64(e.eval_batch(q, SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, (bad[:8], got[bad[:2]], exp[bad[:2]])
        assert {int(r[8]) for r in raw16(q)} == set(range(2, 8))
    finally:
        e.close()
