"""The plain kernels on the split card table (two 8-byte LDS arrays per wave) against the oracle, bit for bit: one batch
of 40 queries -- 2, 3, 6, 9, 10 players x 0, 3, 4, 5 table cards x two hands -- at 2100 runs (three tasks, the last one
partial, lanes beyond `runs` idle), at 300 runs (one-launch kernel, host and device entry), one 20 000-run query (many
waves on one row), both dealing laws, the parity mode on the 2-6 player cells, plain and split-pot rows.  Before the flop
the deck holds 50 cards (every slot pair e, e + 32 of the 8-byte reads is reachable); the turn boards leave 46.

Split-pot rows are checked word for word in their plain part (13 words) and by tie == sum(tie_ways) on every cell (the
oracle has no split-pot mode), and all 22 words against rows derived from the oracle's per-iteration trace
(tests/ways_expect.py) on three cells of the 300-run batch."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import ways_expect as W

pytestmark = pytest.mark.gpu

SEED, MT_SEED, FQ = (1 << 40) | 0xCA2D7AB, 0x13572468, 11
PLAYERS, STREETS = (2, 3, 6, 9, 10), (0, 3, 4, 5)
BOARD = ["9H", "TH", "2S", "2D", "KC"]
HANDS = [["AS", "AD"], ["7C", "3H"]]


def batch(runs, players=PLAYERS):
    hole, board, npl = [], [], []
    for p in players:
        for nb in STREETS:
            for h in HANDS:
                hole.append([npa.card_id(c) for c in h])
                board.append([npa.card_id(c) for c in BOARD[:nb]] + [255] * (5 - nb))
                npl.append(p)
    return npa.pack_queries(hole, board, npl, [runs] * len(npl))


def raw16(q):
    return q.view(np.uint8).reshape(-1, 16)


def u64(r, words=13):
    return np.asarray(r).view(np.uint64).reshape(-1, words)


@pytest.fixture(scope="module")
def want():
    out = {}
    for runs in (2100, 300):
        for name, om in (("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM)):
            out[runs, name] = O.run_batch(om, raw16(batch(runs)), SEED, first_qid=FQ, threads=16)
    out["replay"] = O.run_batch(O.MODE_MT, raw16(batch(2100, (2, 3, 6))), MT_SEED, first_qid=FQ, threads=16)
    big = batch(20000)[16:17]   # 6 players before the flop: a 50-card deck
    out["big"] = O.run_batch(O.MODE_CTR, raw16(big), SEED, first_qid=FQ, threads=16)
    return out


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def check_ways(rows, plain):
    rows = u64(rows, 22)
    assert np.array_equal(rows[:, :13], plain)
    assert np.array_equal(rows[:, 13:].sum(1), rows[:, 3])   # tie = sum of tie_ways


def test_batch_has_the_forty_cells():
    q = raw16(batch(2100))
    assert len(q) == 40 and len({(int(r[8]), int(r[7])) for r in q}) == 20


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_three_tasks_the_last_partial(eng, want, law):
    eng.set_dealing_law(law)
    try:
        q = batch(2100)
        assert np.array_equal(u64(eng.eval_batch(q, SEED, first_query_id=FQ)), want[2100, law])
        check_ways(eng.eval_batch_ways(q, SEED, first_query_id=FQ), want[2100, law])
    finally:
        eng.set_dealing_law("reference")


def test_parity_mode_two_to_six_players(eng, want):
    q = batch(2100, (2, 3, 6))
    got = u64(eng.eval_batch(q, MT_SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
    assert np.array_equal(got, want["replay"])
    check_ways(eng.eval_batch_ways(q, MT_SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937), want["replay"])


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_one_launch_path_and_device_entry(eng, want, law):
    torch = pytest.importorskip("torch")
    eng.set_dealing_law(law)
    try:
        q = batch(300)
        assert np.array_equal(u64(eng.eval_batch(q, SEED, first_query_id=FQ)), want[300, law])
        check_ways(eng.eval_batch_ways(q, SEED, first_query_id=FQ), want[300, law])
        dq = torch.from_numpy(raw16(q).copy()).cuda()
        out = torch.full((len(q), 22), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.eval_batch_device_ways(dq.data_ptr(), len(q), SEED, out.data_ptr(), first_query_id=FQ,
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        check_ways(out.cpu().numpy(), want[300, law])
    finally:
        eng.set_dealing_law("reference")


def test_many_waves_on_one_row(eng, want):
    q = batch(20000)[16:17]
    r = raw16(q)[0]
    assert (int(r[8]), int(r[7])) == (6, 0)
    assert np.array_equal(u64(eng.eval_batch(q, SEED, first_query_id=FQ)), want["big"])
    check_ways(eng.eval_batch_ways(q, SEED, first_query_id=FQ), want["big"])


@pytest.mark.parametrize("cell", [(6, 0, 1), (10, 3, 0), (3, 4, 1)])   # (players, table cards, hand)
def test_tie_ways_words_against_the_trace(eng, cell):
    p, nb, h = cell
    i = (PLAYERS.index(p) * len(STREETS) + STREETS.index(nb)) * len(HANDS) + h
    q = batch(300)
    r = raw16(q)[i]
    assert (int(r[8]), int(r[7])) == (p, nb)
    want_row = W.expected_row(O.MODE_CTR, HANDS[h], BOARD[:nb], p, 300, SEED, FQ + i)
    assert np.array_equal(u64(eng.eval_batch_ways(q, SEED, first_query_id=FQ), 22)[i], want_row)
