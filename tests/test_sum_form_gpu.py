"""The plain kernels in the sum form (rank-sum hash) against the oracle, bit for bit: the 40 (players, street) cells at
8193 runs (bulk kernel, and the sub-task cut when the batch is small) and at 1000 runs (one-launch kernel), both dealing
laws and parity mode, on boards that are paired, tripled and three-suited so that every hand type and the flush / rank
id interleave occur."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = (1 << 41) | 0x51F15EED
MT_SEED = 0x2545F491
FQ = 77
RANKS = "23456789TJQKA"


def cid(s):
    return npa.card_id(s)


BOARDS = {   # street -> boards: paired, tripled, three of a suit, four to a straight flush
    0: [[]],
    3: [["AS", "AD", "7C"], ["9H", "9D", "9C"], ["2S", "8S", "KS"], ["TH", "JH", "QH"]],
    4: [["AS", "AD", "7C", "7D"], ["9H", "9D", "9C", "KS"], ["2S", "8S", "KS", "3D"], ["9H", "TH", "JH", "QH"]],
    5: [["AS", "AD", "7C", "7D", "2H"], ["9H", "9D", "9C", "KS", "KD"], ["2S", "8S", "KS", "3D", "3C"],
        ["9H", "TH", "JH", "QH", "2C"], ["5C", "5D", "5H", "5S", "QD"]],
}


def batch(runs):
    rng = np.random.default_rng(5)
    hole, board, npl = [], [], []
    for p in range(1, 11):
        for nb in (0, 3, 4, 5):
            for b in BOARDS[nb]:
                t = [cid(c) for c in b]
                rest = [c for c in rng.permutation(52) if c not in t]
                hole.append(rest[:2])
                board.append(t + [255] * (5 - nb))
                npl.append(p)
    return npa.pack_queries(hole, board, npl, [runs] * len(npl))


def u64(r):
    return r.view(np.uint64).reshape(-1, 13)


@pytest.fixture(scope="module")
def want():
    out = {}
    for runs in (8193, 1000):
        raw = batch(runs).view(np.uint8).reshape(-1, 16)
        for name, om, seed in (("reference", O.MODE_CTR, SEED), ("uniform", O.MODE_CTR_UNIFORM, SEED), ("replay", O.MODE_MT, MT_SEED)):
            out[runs, name] = O.run_batch(om, raw, seed, first_qid=FQ, threads=16)
    return out


@pytest.mark.parametrize("runs", [8193, 1000])
def test_sum_form_kernels_match_the_oracle(want, runs):
    q = batch(runs)
    assert len({(int(r[8]), int(r[7])) for r in q.view(np.uint8).reshape(-1, 16)}) == 40
    e = npa.Engine(0)
    try:
        for law in ("reference", "uniform"):
            e.set_dealing_law(law)
            assert np.array_equal(u64(e.eval_batch(q, SEED, first_query_id=FQ)), want[runs, law]), law
            for i in (0, len(q) // 2, len(q) - 1):   # a query alone: the cut (8193 runs) / the one-launch kernel (1000)
                got = u64(e.eval_batch(q[i:i + 1], SEED, first_query_id=FQ + i))
                assert np.array_equal(got, want[runs, law][i:i + 1]), (law, i)
        e.set_dealing_law("reference")
        got = u64(e.eval_batch(q, MT_SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
        assert np.array_equal(got, want[runs, "replay"])
    finally:
        e.close()
