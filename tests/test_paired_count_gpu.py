"""The paired count on the device: the straight forms of mcq_iteration_sum count a closed epoch's hole registers two per
popcount (mcq_hole_count2; the host build of the same text: tests/test_paired_count_host.py).

Which shapes count a pair under the shipped rule: the forms whose plan has 14 or more draws.  Such a plan closes an epoch of
eight holes behind the fourth opponent -- its second register is biased while it is still partly filled, by the scan of
draw 6, and scanned biased by draw 7 -- and ten players pass two such pairs; the shorter plans count no pair and stay what
they were.  (A closed biased register that stays partly filled occurs under rules 1 and 2 only: the host test has them.)
The kernels: mcq_eval_kernel in production mode, both laws, cut and uncut, plain and split-pot rows, and its parity
instances with plain rows for 1 to 5 opponents.

One query per cell of 2 to 10 players x 0, 3, 4, 5 table cards, 1041 runs each: one full task of 1024 iterations and a ragged
one of 17.  An engine opened with MCQ_DIRECT_MAX_TASKS=0 sends such queries to the bulk kernel, whose small batches the host
cuts into sub-tasks unless MCQ_SPLIT_MAX=0 as well.

* uncut and cut bulk kernel, each through the host entry and the device-pointer entry, under both dealing laws: == the
  oracle's CTR mode bit for bit;
* split-pot rows on both paths: the plain words == the oracle's, tie_ways == the host build of the lane code;
* parity mode, plain rows, 1 to 5 opponents (and 6, the general form) == the oracle's MT19937 walk bit for bit.
"""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import hostsim_paired

pytestmark = pytest.mark.gpu

SEED, FQ = (1 << 44) | 0x9A1ED, 57
RUNS = 1041
LAWS = [("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM)]
HANDS = [[50, 46], [23, 4], [43, 39], [12, 16]]
BOARD = [28, 32, 5, 3, 45]
CELLS = [(HANDS[(p + nb) % 4], BOARD[:nb], p) for p in range(2, 11) for nb in (0, 3, 4, 5)]
PATHS = {"uncut": {"MCQ_DIRECT_MAX_TASKS": "0", "MCQ_SPLIT_MAX": "0"}, "cut": {"MCQ_DIRECT_MAX_TASKS": "0"}}


def queries(cells=CELLS, runs=RUNS):
    hole = np.array([h for h, _, _ in cells], np.uint8)
    board = np.array([list(b) + [255] * (5 - len(b)) for _, b, _ in cells], np.uint8)
    return npa.pack_queries(hole, board, np.array([p for _, _, p in cells]), runs)


def raw16(q):
    return np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)


def u64(r, words=13):
    return np.ascontiguousarray(r).view(np.uint64).reshape(-1, words)


def form_of(r):
    """the straight form the kernels' dispatch gives a query"""
    nopp, ndeal = int(r[8]) - 1, 5 - int(r[7])
    return nopp, (ndeal if ndeal in (5, 2, 1) and nopp <= 7 else -1)


def host_ways(uniform):
    """the 22-word rows from the host build with the switch as the product ships it"""
    paired = bool(hostsim_paired.shipped_switch())
    out = []
    for i, r in enumerate(raw16(queries())):
        nopp, ndeal = form_of(r)
        out.append(hostsim_paired.rows(r, SEED, FQ + i, nopp, ndeal, uniform=uniform, ways=True, paired=paired)[0])
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
    q = raw16(queries())
    assert len(q) == 36 and len({(int(r[8]), int(r[7])) for r in q}) == 36
    assert RUNS == 1024 + 17 and all(int(r[12:16].view("<u4")[0]) == RUNS for r in q)
    for r in q:
        assert len(set(r[0:2].tolist()) | set(r[2:2 + int(r[7])].tolist())) == 2 + int(r[7])      # no card twice
    kinds = {}
    for r in q:                                              # what the plan of every cell's form pairs
        nopp, ndeal = form_of(r)
        pl = hostsim_paired.plan(2 * nopp + (ndeal if ndeal >= 0 else 5), 3)
        kinds[(int(r[8]), int(r[7]))] = (pl["regs"], pl["holes"], pl["cost"] - pl["cost_paired"], 2 * nopp + (ndeal if ndeal >= 0 else 5))
    assert kinds[(10, 0)][0][:4] == [0, 2, 0, 2] and kinds[(10, 0)][2] == 22                       # two full pairs
    assert kinds[(6, 0)][0][:3] == [0, 2, 0] and kinds[(6, 0)][2] == 7                             # the flagship shape
    assert all((k[2] > 0) == (k[3] >= 14) for k in kinds.values())
    assert sum(k[2] > 0 for k in kinds.values()) >= 16 and sum(k[2] == 0 for k in kinds.values()) >= 12
    assert all(kinds[(p, nb)][2] > 0 for p in (8, 9, 10) for nb in (0, 3, 4, 5))
    for law, _ in LAWS:
        assert np.array_equal(want[law]["ways"][:, :13], want[law]["plain"])     # the host build itself against the oracle
        assert want[law]["ways"][:, 14:].any()                                   # pots shared three ways and more occur


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
            rows = u64(e.eval_batch_ways(q, SEED, first_query_id=FQ), 22)
            bad = np.flatnonzero((rows != ways).any(1))
            assert len(bad) == 0, (law, "ways", bad[:8], rows[bad[:2]], ways[bad[:2]])
            assert np.array_equal(on_device(e.eval_batch_device_ways, q, 22), ways), (law, "device ways")
            for i in (16, 24, 32, 35):                                           # one query alone in its call
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
