"""Split-pot tallies on the GPU: mcq_eval_batch_ways / mcq_eval_batch_device_ways, bit for bit against rows derived from
the oracle's per-iteration trace (tests/ways_expect.py), in the three regimes that hit every new kernel instantiation,
under both dealing laws and in parity mode."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import montecarlo_hip as mh
from oracle import oracle as O
from tests import hostsim_ways as H
from tests import ways_expect as W

pytestmark = pytest.mark.gpu

# (oracle mode, library mode, dealing law)
FRONTS = [(O.MODE_CTR, npa.MODE_PHILOX, "reference"), (O.MODE_CTR_UNIFORM, npa.MODE_PHILOX, "uniform"),
          (O.MODE_MT, npa.MODE_REPLAY_MT19937, "reference")]
BULK_RUNS = 9000      # nine tasks: above the one-launch path's eight, so the priced path with the evaluation kernel


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0, kernel_times=True)
    yield e
    e.set_dealing_law("reference")
    e.close()


def w64(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 22)


def board5(board):
    return np.array([[npa.card_id(c) for c in board] + [255] * (5 - len(board))], np.uint8)


def hero2(hero):
    return np.array([[npa.card_id(c) for c in hero]], np.uint8)


def cases(runs):
    return np.concatenate([npa.pack_queries(hero2(h), board5(b), n, runs) for h, b, n in W.CASES])


def random_small(g, B):
    """mixed small queries: 2..10 players, every street, 200..2000 iterations"""
    hole = np.zeros((B, 2), np.uint8)
    board = np.full((B, 5), 255, np.uint8)
    for i in range(B):
        nb = int(g.choice([0, 3, 4, 5]))
        c = g.permutation(52)[:2 + nb]
        hole[i] = c[:2]
        board[i, :nb] = c[2:]
    return npa.pack_queries(hole, board, g.integers(2, 11, B).astype(np.uint8), g.integers(200, 2001, B).astype(np.uint32))


def raw16(q):
    return np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)


def check_invariants(rows, q):
    assert np.array_equal(rows[:, 13:].sum(1), rows[:, 3])
    npl = raw16(q)[:, 8].astype(int)
    for k in range(2, 11):
        assert not rows[npl < k, 13 + k - 2].any()


@pytest.mark.parametrize("omode,mode,law", FRONTS)
def test_one_small_query_takes_the_one_launch_kernel(eng, omode, mode, law):
    eng.set_dealing_law(law)
    exp = [W.expected_case(omode, i) for i in range(len(W.CASES))]
    W.assert_cases_vary(exp)
    q = cases(W.RUNS)
    for i in range(len(W.CASES)):
        got = w64(eng.eval_batch_ways(q[i:i + 1], W.SEED, first_query_id=W.QID, mode=mode))[0]
        assert np.array_equal(got, exp[i]), (i, got, exp[i])
        plain = eng.eval_batch(q[i:i + 1], W.SEED, first_query_id=W.QID, mode=mode)
        assert got[:13].tobytes() == plain.tobytes()


@pytest.mark.parametrize("omode,mode,law", FRONTS)
def test_batch_of_1024_mixed_small_queries(eng, omode, mode, law):
    eng.set_dealing_law(law)
    q = random_small(np.random.default_rng(77), 1024)
    q[:len(W.CASES)] = cases(W.RUNS)
    first = W.QID          # query i of the batch runs under id QID + i: row 0 is case 0 under (SEED, QID)
    got = w64(eng.eval_batch_ways(q, W.SEED, first_query_id=first, mode=mode))
    exp0 = W.expected_case(omode, 0)
    assert np.array_equal(got[0], exp0)
    for i in range(1, len(W.CASES)):
        h, b, n = W.CASES[i]
        assert np.array_equal(got[i], W.expected_row(omode, h, b, n, W.RUNS, W.SEED, first + i)), i
    for i in range(len(q)):   # every row against the host walk of the same lane code (pinned to the trace by the host tests)
        assert np.array_equal(got[i], H.run(omode, raw16(q)[i], W.SEED, first + i, general=True)), i
    check_invariants(got, q)
    plain = eng.eval_batch(q, W.SEED, first_query_id=first, mode=mode)
    assert np.ascontiguousarray(got[:, :13]).tobytes() == plain.tobytes()
    # a batch split in two calls with matching first_query_id
    a = w64(eng.eval_batch_ways(q[:400], W.SEED, first_query_id=first, mode=mode))
    b = w64(eng.eval_batch_ways(q[400:], W.SEED, first_query_id=first + 400, mode=mode))
    assert np.array_equal(np.concatenate([a, b]), got)


@pytest.mark.parametrize("omode,mode,law", FRONTS)
def test_runs_above_8192_take_the_bulk_kernel_and_the_sub_task_cut(eng, omode, mode, law):
    eng.set_dealing_law(law)
    q = cases(BULK_RUNS)
    exp = np.stack([W.expected_row(omode, h, b, n, BULK_RUNS, W.SEED, W.QID + i) for i, (h, b, n) in enumerate(W.CASES)])
    W.assert_cases_vary(exp)
    got = w64(eng.eval_batch_ways(q, W.SEED, first_query_id=W.QID, mode=mode))      # 63 tasks: cut into sub-tasks
    assert np.array_equal(got, exp), (got, exp)
    plain = eng.eval_batch(q, W.SEED, first_query_id=W.QID, mode=mode)
    assert np.ascontiguousarray(got[:, :13]).tobytes() == plain.tobytes()
    # many such queries: more tasks than the cut is made for -- the bulk instantiation proper
    g = np.random.default_rng(5)
    B = 400
    big = np.concatenate([q, npa.pack_queries(np.array([g.permutation(52)[:2] for _ in range(B)], np.uint8),
                                              np.full((B, 5), 255, np.uint8), g.integers(2, 11, B).astype(np.uint8), BULK_RUNS)])
    gb = w64(eng.eval_batch_ways(big, W.SEED, first_query_id=W.QID, mode=mode))
    assert np.array_equal(gb[:len(q)], exp)
    for i in range(len(q), len(big), 7):
        assert np.array_equal(gb[i], H.run(omode, raw16(big)[i], W.SEED, W.QID + i)), i
    check_invariants(gb, big)
    assert np.ascontiguousarray(gb[:, :13]).tobytes() == eng.eval_batch(big, W.SEED, first_query_id=W.QID, mode=mode).tobytes()
    half = len(big) // 2
    parts = [w64(eng.eval_batch_ways(big[:half], W.SEED, first_query_id=W.QID, mode=mode)),
             w64(eng.eval_batch_ways(big[half:], W.SEED, first_query_id=W.QID + half, mode=mode))]
    assert np.array_equal(np.concatenate(parts), gb)


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_more_rows_than_the_publish_path_takes(eng, law):
    """above 8192 rows the host entry copies the rows back instead of publishing them through pinned memory"""
    eng.set_dealing_law(law)
    g = np.random.default_rng(6)
    B = 8300
    q = npa.pack_queries(np.array([g.permutation(52)[:2] for _ in range(B)], np.uint8), np.full((B, 5), 255, np.uint8),
                         g.integers(2, 5, B).astype(np.uint8), BULK_RUNS)
    got = w64(eng.eval_batch_ways(q, 11, first_query_id=5))
    check_invariants(got, q)
    assert np.ascontiguousarray(got[:, :13]).tobytes() == eng.eval_batch(q, 11, first_query_id=5).tobytes()
    omode = O.MODE_CTR_UNIFORM if law == "uniform" else O.MODE_CTR
    for i in range(0, B, 83):
        assert np.array_equal(got[i], H.run(omode, raw16(q)[i], 11, 5 + i)), i
    again = w64(eng.eval_batch_ways(q[:64], 11, first_query_id=5))     # the rows in HBM were left clean
    assert np.array_equal(again, got[:64])


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_device_entry_equals_the_host_entry_and_marks_invalid_queries(eng, law):
    torch = pytest.importorskip("torch")
    eng.set_dealing_law(law)
    g = np.random.default_rng(8)
    for q in (np.concatenate([cases(W.RUNS), random_small(g, 300)]),                       # cut by the prep kernel
              np.concatenate([cases(BULK_RUNS), random_small(g, 1500)])):                   # more than 1024: never cut
        want = w64(eng.eval_batch_ways(q, W.SEED, first_query_id=W.QID))
        raw = raw16(q).copy()
        bad = [3, len(q) - 1]
        raw[bad[0], 1] = raw[bad[0], 0]        # hero holds the same card twice
        raw[bad[1], 8] = 11                    # eleven players
        dq = torch.from_numpy(raw).cuda()
        out = torch.full((len(q), 22), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.eval_batch_device_ways(dq.data_ptr(), len(q), W.SEED, out.data_ptr(), first_query_id=W.QID,
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        ok = np.ones(len(q), bool)
        ok[bad] = False
        assert np.array_equal(got[ok], want[ok])
        for i in bad:
            assert got[i, 0] == 0 and got[i, 1] == 2 ** 64 - 1 and not got[i, 2:].any(), got[i]


def test_host_entry_einval_leaves_out_untouched(eng):
    eng.set_dealing_law("reference")
    q = cases(1000)
    q["hole"][2] = [7, 7]
    out = np.full(len(q) * 22, 0xA5A5A5A5A5A5A5A5, np.uint64)
    L = npa.load_library()
    rc = L.mcq_eval_batch_ways(eng._ctx, q.ctypes.data, len(q), 1, 0, npa.MODE_PHILOX, out.ctypes.data)
    assert rc == -1 and (out == 0xA5A5A5A5A5A5A5A5).all()
    with pytest.raises(ValueError):
        eng.eval_batch_ways(q, 1)
    with pytest.raises(ValueError):
        eng.eval_batch_ways(cases(1000), 1, mode=7)


def test_sanity_against_arithmetic(eng):
    eng.set_dealing_law("reference")
    g = np.random.default_rng(9)
    hole = np.array([g.permutation(52)[:2] for _ in range(256)], np.uint8)
    none = np.full((256, 5), 255, np.uint8)
    for runs in (1000, 20000):
        hu = w64(eng.eval_batch_ways(npa.pack_queries(hole, none, 2, runs), 3))
        assert np.array_equal(hu[:, 13], hu[:, 3]) and not hu[:, 14:].any() and hu[:, 3].any()    # heads-up: every tie is two-way
        alone = w64(eng.eval_batch_ways(npa.pack_queries(hole, none, 1, runs), 3))
        assert (alone[:, 2] == runs).all() and not alone[:, 3].any() and not alone[:, 13:].any()


def test_python_surface(eng):
    """get_equity_batch(ties='split'), get_pot_equity, pot_share and the torch op against the host entry."""
    eng.set_dealing_law("reference")
    q = cases(W.RUNS)
    rows = eng.eval_batch_ways(q, W.SEED, first_query_id=W.QID)
    t = w64(rows).astype(np.float64)
    formula = (t[:, 2] + sum(t[:, 13 + k - 2] / k for k in range(2, 11))) / t[:, 0]
    assert np.allclose(npa.pot_share(rows), formula, rtol=0, atol=1e-15)
    credited = (t[:, 2] + t[:, 3]) / t[:, 0]
    assert (npa.pot_share(rows) <= credited).all() and (npa.pot_share(rows) < credited).any()
    raw = raw16(q)
    eq, tal = mh.get_equity_batch(raw[:, 0:2], np.where(np.arange(5)[None, :] < raw[:, 7:8], raw[:, 2:7], 255), raw[:, 8], W.RUNS,
                                  seed=W.SEED, first_query_id=W.QID, engine=eng, ties="split")
    assert tal.shape == (len(q), 22) and np.array_equal(tal, w64(rows)) and np.array_equal(eq, npa.pot_share(rows))
    eq0, tal0 = mh.get_equity_batch(raw[:, 0:2], np.where(np.arange(5)[None, :] < raw[:, 7:8], raw[:, 2:7], 255), raw[:, 8],
                                    W.RUNS, seed=W.SEED, first_query_id=W.QID, engine=eng)
    assert tal0.shape == (len(q), 13) and np.array_equal(tal0, w64(rows)[:, :13]) and np.array_equal(eq0, credited)
    # get_pot_equity: the same stream state as get_equity (one query id per call)
    mh.configure(mode="philox")
    mh.seed(41)
    a = [mh.get_pot_equity({"7C", "2D"}, set(), 10, 4096), mh.get_pot_equity(["AC", "QD"], ["AD", "AH", "KS"], 4, 4096)]
    d = npa.default_engine()
    want = [float(npa.pot_share(d.eval_batch_ways(cases(4096)[1:2], 41, first_query_id=0))[0]),
            float(npa.pot_share(d.eval_batch_ways(cases(4096)[5:6], 41, first_query_id=1))[0])]
    assert a == want
    mh.seed(41)
    assert mh.get_equity({"7C", "2D"}, set(), 10, 4096) > a[0]        # ties credited in full
    torch = pytest.importorskip("torch")
    from neuron_poker_amd import torch_ops
    with pytest.raises(ValueError):
        torch_ops.get_equity_batch_torch(torch.zeros((1, 2), dtype=torch.uint8), torch.zeros((1, 5), dtype=torch.uint8), 2, 10,
                                         ties="bogus")
    hole_t = torch.from_numpy(raw[:, 0:2].copy()).cuda()
    board_t = torch.from_numpy(np.where(np.arange(5)[None, :] < raw[:, 7:8], raw[:, 2:7], 255).astype(np.uint8)).cuda()
    npl_t = torch.from_numpy(raw[:, 8].copy()).cuda()
    eq_t, tal_t = torch_ops.get_equity_batch_torch(hole_t, board_t, npl_t, W.RUNS, seed=W.SEED, first_query_id=W.QID, engine=eng,
                                                   ties="split")
    assert tal_t.is_cuda and eq_t.is_cuda and tuple(tal_t.shape) == (len(q), 22)
    assert np.array_equal(tal_t.cpu().numpy().view(np.uint64), w64(rows))
    assert np.allclose(eq_t.cpu().numpy(), npa.pot_share(rows), rtol=0, atol=1e-15)


def test_device_entry_inside_a_hip_graph(eng):
    """As the plain device entry (tests/test_gpu_parity.py): one ordinary call on the stream, then capture and replay."""
    torch = pytest.importorskip("torch")
    eng.set_dealing_law("reference")
    q = np.concatenate([cases(1500), random_small(np.random.default_rng(12), 377)])
    B = len(q)
    want = w64(eng.eval_batch_ways(q, 424242, first_query_id=9))
    d_q = torch.from_numpy(raw16(q).copy()).cuda()
    out = torch.zeros((B, 22), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.eval_batch_device_ways(d_q.data_ptr(), B, 1, out.data_ptr(), first_query_id=0, stream=s.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        eng.eval_batch_device_ways(d_q.data_ptr(), B, 424242, out.data_ptr(), first_query_id=9,
                                   stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
