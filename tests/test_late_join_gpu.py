"""The late join of an opponent pair on the device: in mcq_iteration_sum's straight forms a pair's hand is put together
behind the NEXT pair's reads (the last pair's behind the table's draws), held there by an empty asm that only a device
build sees (the host build of the same text: tests/test_late_join_host.py).

Which kernels run those forms, and so carry the join: mcq_eval_kernel in production mode, both laws, cut and uncut, plain and
split-pot rows (1 to 9 opponents), and its parity instances with plain rows for 1 to 5 opponents.  The one-launch kernel
(mcq_eval_direct_kernel), parity mode with split-pot rows and parity mode with six or more opponents run the general form,
which keeps the old order: their cases here are regression checks of object code the join does not alter.

One query per cell of 2 to 10 players x 0, 3, 4, 5 table cards, and four cells picked by hand: a hero holding the two
highest cards of the deck, a table that holds the deck's top card, ten players on an empty table (twenty holes: all five
registers full) and two players on a full table (no scan of a full register at all).

* 16 384 + 17 runs each and one further query of 100 000 runs: above the one-launch path's eight tasks, with a ragged last
  task.  That batch is 778 tasks, which the host cuts into sub-tasks (mcq_pick_split through mcq_plan_geometry,
  csrc/mcq_plan.hpp, held to its mirror by tests/test_plan_host.py: up to 8 x 256 CUs / 2) -- the small-batch cut of the
  bulk kernel; the batch twice over is 1 556 tasks and runs uncut -- the bulk instance proper.
* the same cells at 1 000 runs: the one-launch kernel (general form, see above).
* under both dealing laws: Engine.eval_batch == the oracle's CTR mode bit for bit; Engine.eval_batch_ways: its plain row ==
  eval_batch byte for byte, its tie_ways == the host build of the lane code; the device-pointer entries == the host entries.
* parity mode at 129 and 4 500 runs on eight of the cells == the oracle's MT19937 mode bit for bit: 1, 2, 3, 4 and 5
  opponents take the straight forms with the join (plain rows), 6 opponents the general form.
"""
import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import hostsim_join

pytestmark = pytest.mark.gpu

SEED, FQ = (1 << 44) | 0x7A7E, 9
BULK_RUNS, SMALL_RUNS, LONG_RUNS = 16384 + 17, 1000, 100000
PARITY_RUNS = (129, 4500)
LAWS = [("reference", O.MODE_CTR), ("uniform", O.MODE_CTR_UNIFORM)]
HANDS = [[48, 44], [21, 6], [45, 41], [14, 18]]          # AC KC, 7D 3H, KD QD, 5H 6H
BOARD = [30, 34, 3, 1, 47]                                # 9H TH 2S 2D KS
GRID = [(HANDS[(p + nb) % 4], BOARD[:nb], p) for p in range(2, 11) for nb in (0, 3, 4, 5)]
EDGES = [([51, 50], [], 6),                               # hero holds the two highest cards of the deck
         ([0, 5], [51, 20, 33], 4),                       # the table holds the deck's top card
         ([0, 1], [], 10),                                # twenty holes: all five registers full
         ([13, 26], [4, 9, 19, 36, 49], 2)]               # one opponent, nothing to come
CELLS = GRID + EDGES
# 2, 3, 4, 5, 6 players: 1 to 5 opponents, the straight parity forms; 7 players: the general form; the edge cells: 5 and 3
PARITY_CELLS = [GRID[0], GRID[5], GRID[9], GRID[14], GRID[18], GRID[23], EDGES[0], EDGES[1]]


def pack(cells, runs):
    hole = np.array([h for h, _, _ in cells], np.uint8)
    board = np.array([list(b) + [255] * (5 - len(b)) for _, b, _ in cells], np.uint8)
    return npa.pack_queries(hole, board, np.array([p for _, _, p in cells]), runs)


def bulk_batch():
    return np.concatenate([pack(CELLS, BULK_RUNS), pack([GRID[16]], LONG_RUNS)])    # the long one: 6-max before the flop


def raw16(q):
    return np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)


def u64(r, words=13):
    return np.ascontiguousarray(r).view(np.uint64).reshape(-1, words)


def tasks(q):
    return [(int(r[12:16].view("<u4")[0]) + 1023) // 1024 for r in raw16(q)]


def host_ways(q, first_qid, uniform):
    """the 22-word rows from the host build, each query through the instantiation the kernels' dispatch gives it"""
    out = []
    for i, r in enumerate(raw16(q)):
        nopp, ndeal = int(r[8]) - 1, 5 - int(r[7])
        ndeal = ndeal if ndeal in (5, 2, 1) and nopp <= 7 else -1
        out.append(hostsim_join.rows(r, SEED, first_qid + i, nopp, ndeal, uniform=uniform, ways=True)[0])
    return np.stack(out)


@pytest.fixture(scope="module")
def want():
    """per law: the oracle's rows of the bulk batch twice over and of the small batch, and the host build's 22-word rows of
    the bulk batch and the small batch -- computed once, read-only"""
    two, small = np.concatenate([bulk_batch(), bulk_batch()]), pack(CELLS, SMALL_RUNS)
    out = {}
    for law, omode in LAWS:
        w = {"two": O.run_batch(omode, raw16(two), SEED, first_qid=FQ, threads=16),
             "small": O.run_batch(omode, raw16(small), SEED, first_qid=FQ, threads=16),
             "ways_bulk": host_ways(bulk_batch(), FQ, law == "uniform"),
             "ways_small": host_ways(small, FQ, law == "uniform")}
        for v in w.values():
            v.setflags(write=False)
        out[law] = w
    return out


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.set_dealing_law("reference")
    e.close()


def test_batches_take_the_paths_they_claim():
    q = raw16(bulk_batch())
    assert len(q) == 41 and len({(int(r[8]), int(r[7])) for r in q[:36]}) == 36
    t = tasks(q)
    assert min(t) > 8 and t[0] == 17 and BULK_RUNS % 1024 == 17 and t[-1] == 98      # never the one-launch path
    assert 2 * sum(t) <= 8 * 256 and 2 * max(t) <= 512                               # cut once by mcq_pick_split on 256 CUs
    assert 2 * (2 * sum(t)) > 8 * 256                                                # the batch twice over: uncut
    assert max(tasks(pack(CELLS, SMALL_RUNS))) == 1
    assert {(p, len(b)) for _, b, p in CELLS} >= {(10, 0), (2, 5)}
    assert sorted(EDGES[0][0]) == [50, 51] and 51 in EDGES[1][1]


@pytest.mark.parametrize("law,omode", LAWS)
def test_bulk_kernel_cut_and_uncut(eng, want, law, omode):
    eng.set_dealing_law(law)
    w = want[law]["two"]
    one, n = bulk_batch(), len(bulk_batch())
    got = u64(eng.eval_batch(one, SEED, first_query_id=FQ))
    bad = np.flatnonzero((got != w[:n]).any(1))
    assert len(bad) == 0, (bad[:8], got[bad[:2]], w[bad[:2]])
    got2 = u64(eng.eval_batch(np.concatenate([one, one]), SEED, first_query_id=FQ))
    bad = np.flatnonzero((got2 != w).any(1))
    assert len(bad) == 0, (bad[:8], got2[bad[:2]], w[bad[:2]])


@pytest.mark.parametrize("law,omode", LAWS)
def test_bulk_kernel_split_pot_rows(eng, want, law, omode):
    eng.set_dealing_law(law)
    one, n = bulk_batch(), len(bulk_batch())
    hw = want[law]["ways_bulk"]
    assert np.array_equal(hw[:, :13], want[law]["two"][:n])       # the host build itself against the oracle
    assert hw[:, 14:].any()                                        # pots shared three ways and more occur
    for q, first in ((one, FQ), (np.concatenate([one, one]), FQ)):
        rows = eng.eval_batch_ways(q, SEED, first_query_id=first)
        plain = eng.eval_batch(q, SEED, first_query_id=first)
        r = u64(rows, 22)
        assert np.ascontiguousarray(r[:, :13]).tobytes() == plain.tobytes()
        assert np.array_equal(r[:n], hw), np.flatnonzero((r[:n] != hw).any(1))[:8]
        assert np.array_equal(r[:, :13], want[law]["two"][:len(q)])
        assert np.array_equal(r[:, 13:].sum(1), r[:, 3])


@pytest.mark.parametrize("law,omode", LAWS)
def test_one_launch_kernel(eng, want, law, omode):
    eng.set_dealing_law(law)
    q = pack(CELLS, SMALL_RUNS)
    got = u64(eng.eval_batch(q, SEED, first_query_id=FQ))
    assert np.array_equal(got, want[law]["small"]), np.flatnonzero((got != want[law]["small"]).any(1))[:8]
    rows = eng.eval_batch_ways(q, SEED, first_query_id=FQ)
    assert np.ascontiguousarray(u64(rows, 22)[:, :13]).tobytes() == eng.eval_batch(q, SEED, first_query_id=FQ).tobytes()
    assert np.array_equal(u64(rows, 22), want[law]["ways_small"])
    for i in (0, 16, 35, 36, 38):                                  # one query alone in its call
        assert np.array_equal(u64(eng.eval_batch(q[i:i + 1], SEED, first_query_id=FQ + i))[0], want[law]["small"][i]), i


@pytest.mark.parametrize("runs", PARITY_RUNS)
def test_parity_mode(eng, runs):
    eng.set_dealing_law("reference")
    q = pack(PARITY_CELLS, runs)
    exp = O.run_batch(O.MODE_MT, raw16(q), SEED, first_qid=FQ, threads=8)
    got = u64(eng.eval_batch(q, SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937))
    assert np.array_equal(got, exp), (got, exp)
    rows = u64(eng.eval_batch_ways(q, SEED, first_query_id=FQ, mode=npa.MODE_REPLAY_MT19937), 22)
    assert np.array_equal(rows[:, :13], exp)
    assert np.array_equal(rows[:, 13:].sum(1), rows[:, 3])


@pytest.mark.parametrize("law,omode", LAWS)
def test_device_pointer_entries_equal_the_host_entries(eng, want, law, omode):
    import torch
    eng.set_dealing_law(law)
    one = bulk_batch()
    stream = torch.cuda.current_stream().cuda_stream
    for q, key in ((one, "two"), (np.concatenate([one, one]), "two"), (pack(CELLS, SMALL_RUNS), "small")):
        dq = torch.from_numpy(raw16(q).copy()).cuda()
        out = torch.full((len(q), 13), -1, dtype=torch.int64, device="cuda")
        outw = torch.full((len(q), 22), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.eval_batch_device(dq.data_ptr(), len(q), SEED, out.data_ptr(), first_query_id=FQ, stream=stream)
        eng.eval_batch_device_ways(dq.data_ptr(), len(q), SEED, outw.data_ptr(), first_query_id=FQ, stream=stream)
        torch.cuda.synchronize()
        got, gotw = out.cpu().numpy().view(np.uint64), outw.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want[law][key][:len(q)])
        assert got.tobytes() == eng.eval_batch(q, SEED, first_query_id=FQ).tobytes()
        assert gotw.tobytes() == eng.eval_batch_ways(q, SEED, first_query_id=FQ).tobytes()
    dq = torch.from_numpy(raw16(pack(CELLS, SMALL_RUNS)).copy()).cuda()       # the one-launch device entry
    out = torch.full((len(CELLS), 13), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.eval_batch_device_small(dq.data_ptr(), len(CELLS), SEED, out.data_ptr(), first_query_id=FQ, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want[law]["small"])
