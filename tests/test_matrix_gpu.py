"""mcq_exact_matrix on the GPU: the kernels' matrices against the host build of the same lane code bit for bit, the full
flop against entries that know nothing of the matrix (row sums = the hero-range rows, weighted row sums = the weighted rows,
single entries = the all-in enumeration of the two hands), and the conventions of an entry (determinism, batch and chunk
invariance, the device entry, refusals)."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import matrix_cases as MC

pytestmark = pytest.mark.gpu
ROWS = MC.ROWS


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


_gpu = {}


def gpu(eng, name):
    """The engine's (win, tie, total) of a case alone, computed once and left unchanged."""
    if name not in _gpu:
        win, tie, total = eng.exact_matrix(MC.record(name))
        win.setflags(write=False)
        tie.setflags(write=False)
        _gpu[name] = (win[0], tie[0], int(total[0]))
    return _gpu[name]


def assert_batch_is_the_host_build(e, names):
    win, tie, total = e.exact_matrix(MC.records(names))
    for i, name in enumerate(names):
        want_w, want_t, want_total = MC.host(name)
        assert int(total[i]) == want_total, name
        assert np.array_equal(win[i], want_w) and np.array_equal(tie[i], want_t), name
        MC.check_shape(name, win[i], tie[i], int(total[i]))
    return win, tie, total


# ---- 1. a mixed batch against the host build, on a fresh engine and with one block walking everything
@pytest.mark.parametrize("cap", [None, 1])
def test_mixed_batch_equals_the_host_build(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("MCQ_EXACT_CU", raising=False)
    else:
        monkeypatch.setenv("MCQ_EXACT_CU", str(cap))
    e = npa.Engine(0)
    try:
        assert_batch_is_the_host_build(e, MC.BATCH)
    finally:
        e.close()


# ---- 2. batch and chunk invariance, determinism
def test_a_batch_is_its_records_alone_and_two_calls_agree(eng, monkeypatch):
    win, tie, total = eng.exact_matrix(MC.records(MC.BATCH))
    again = eng.exact_matrix(MC.records(MC.BATCH))
    assert all(np.array_equal(a, b) for a, b in zip((win, tie, total), again))
    for i, name in enumerate(MC.BATCH):
        w1, t1, tot1 = gpu(eng, name)
        assert np.array_equal(win[i], w1) and np.array_equal(tie[i], t1) and int(total[i]) == tot1, name
    monkeypatch.setenv("MCQ_MATRIX_CHUNK", "2")          # the batch of five in launches of 2, 2 and 1 records
    e = npa.Engine(0)
    try:
        cut = e.exact_matrix(MC.records(MC.BATCH))
    finally:
        e.close()
    assert all(np.array_equal(a, b) for a, b in zip((win, tie, total), cut))


# ---- 3. the full flop against code that knows nothing of the matrix
def _hero_range_records(name, ghost=None):
    board = MC.CASES[name][0]
    q = _lib.pack_query_one([0, 0], board, 2, 1)
    x = _lib.pack_query_ext(1, ghost=ghost, hero_range=_lib.ALL_CLASSES, opp_range=None)
    return q, x


def test_flop_full_row_sums_are_the_hero_range_rows(eng):
    win, tie, total = gpu(eng, "flop_full")
    MC.check_shape("flop_full", win, tie, total)
    rows, _ = eng.exact_hero_range(*_hero_range_records("flop_full"), law="uniform")
    r = rows[0]
    idx = np.array([_lib.hand_index(*h) for h in MC.hands("flop_full")])
    assert len(idx) == 1176 and total == 990
    assert np.array_equal(win.astype(np.uint64).sum(1), r["win"]) and np.array_equal(tie.astype(np.uint64).sum(1), r["tie"])
    apart = 47 * 46 // 2                                  # the hands that share no card with a given hand of D
    assert (r["runs"][idx] == total * apart).all() and r["runs"].sum() == 1176 * total * apart
    assert np.array_equal(MC.meet_mask("flop_full").sum(1)[idx], np.full(1176, apart))


def test_flop_full_weighted_row_sums_are_the_weighted_rows(eng):
    """The matrix is the linear map of the weighted entry: its rows times any opponent table."""
    win, tie, _ = gpu(eng, "flop_full")
    rng = np.random.RandomState(20)
    ow = rng.randint(0, 65536, size=(1, ROWS)).astype(np.uint16)
    ow[0, rng.permutation(ROWS)[:200]] = 0
    ow[0, :2] = 65535, 1
    assert (ow == 0).sum() >= 198 and ow.max() == 65535 and ow[ow > 0].min() == 1
    rows, _ = eng.exact_hero_range_weighted(*_hero_range_records("flop_full"), ow)
    r = rows[0]
    w64 = ow[0].astype(np.uint64)
    assert np.array_equal((win.astype(np.uint64) * w64).sum(1), r["win"])
    assert np.array_equal((tie.astype(np.uint64) * w64).sum(1), r["tie"])
    assert r["win"].max() > 2 ** 32


def _pairs(name, n, seed):
    """n disjoint ordered pairs of hands of D: the corners of the tile grid first -- the hands with the lowest and the highest
    index, pairs out of the first and the last tile row and column --, then a seeded draw."""
    hs = MC.hands(name)
    tile = 64
    last0 = len(hs) // tile * tile if len(hs) % tile else len(hs) - tile
    first, last = hs[:tile], hs[last0:]

    def apart(h, pool):
        return next(g for g in pool if not set(g) & set(h))
    # (the hands of the last tile all hold D's highest card: no two of them can meet)
    out = [(hs[0], apart(hs[0], last[::-1])), (hs[-1], apart(hs[-1], first)), (hs[0], apart(hs[0], first[1:])),
           (first[-1], apart(first[-1], last)), (last[0], apart(last[0], first[::-1])), (hs[-1], apart(hs[-1], hs[last0 - 1::-1]))]
    rng = np.random.RandomState(seed)
    while len(out) < n:
        i, j = rng.randint(0, len(hs), 2)
        if not set(hs[i]) & set(hs[j]):
            out.append((hs[i], hs[j]))
    return out


def _assert_entries_are_the_all_in_enumeration(eng, name, ghost):
    win, tie, total = gpu(eng, name)
    board = MC.CASES[name][0]
    pairs = _pairs(name, 256, 31)
    hole = np.array([h for h, _ in pairs], np.uint8)
    b = np.full((len(pairs), 5), 255, np.uint8)
    b[:, :len(board)] = board
    q = _lib.pack_queries(hole, b, 2, 1)
    x = _lib.pack_query_ext(len(pairs), ghost=ghost)
    x["n_known"] = 1
    x["known"]["cards"][:, 0] = np.array([g for _, g in pairs], np.uint8)
    rows = eng.exact_seats(q, x, law="uniform")
    hi = np.array([_lib.hand_index(*h) for h, _ in pairs])
    gi = np.array([_lib.hand_index(*g) for _, g in pairs])
    assert np.array_equal(rows["seat"]["win"][:, 0], win[hi, gi]) and np.array_equal(rows["seat"]["tie"][:, 0], tie[hi, gi])
    assert np.array_equal(rows["seat"]["win"][:, 1], win[gi, hi]) and (rows["runs"] == total).all()
    assert (tie[hi, gi] > 0).any() and (win[hi, gi] > 0).any() and (win[gi, hi] > 0).any()


def test_flop_full_entries_are_the_all_in_enumeration_of_the_two_hands(eng):
    _assert_entries_are_the_all_in_enumeration(eng, "flop_full", None)


# ---- 4. ... and a turn, its two dead cards given as the records' ghost cards
def test_turn_entries_are_the_all_in_enumeration_with_ghost_cards(eng):
    dead = MC.CASES["turn_dead2"][1]
    assert len(dead) == 2
    _assert_entries_are_the_all_in_enumeration(eng, "turn_dead2", dead)


# ---- 5. structure
@pytest.mark.parametrize("name", list(MC.CASES))
def test_structure(eng, name):
    win, tie, total = gpu(eng, name)
    MC.check_shape(name, win, tie, total)
    MC.check_structure(name, win, tie, total)


# ---- 6. without the tie matrix
def test_without_tie_the_win_matrix_is_the_same(eng):
    names = ["turn_dead2", "flop_tiny"]
    win, tie, total = eng.exact_matrix(MC.records(names), want_tie=False)
    assert tie is None
    for i, name in enumerate(names):
        assert np.array_equal(win[i], gpu(eng, name)[0]) and int(total[i]) == gpu(eng, name)[2]


# ---- 7. the device entry, through the torch op on a stream of its own
def test_device_entry_gives_the_host_entry_s_bytes(eng):
    import torch
    from neuron_poker_amd import torch_ops
    names = ["river", "flop_tiny", "turn_dead2"]
    boards = np.full((len(names), 5), 255, np.uint8)
    dead = np.zeros(len(names), np.int64)
    for i, name in enumerate(names):
        board, gone = MC.CASES[name][:2]
        boards[i, 5 - len(board):] = board                # (empty slots in front: the op left-packs)
        dead[i] = sum(1 << c for c in gone)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        win, tie, total = torch_ops.get_equity_matrix_torch(torch.from_numpy(boards).cuda(), torch.from_numpy(dead), engine=eng)
        only_win, none, _ = torch_ops.get_equity_matrix_torch(torch.from_numpy(boards), torch.from_numpy(dead).cuda(), engine=eng,
                                                              want_tie=False)
    stream.synchronize()
    assert win.is_cuda and tie.is_cuda and win.dtype == torch.int16 and tuple(win.shape) == (len(names), ROWS, ROWS) and none is None
    w, t, w1 = (x.cpu().numpy().view(np.uint16) for x in (win, tie, only_win))
    for i, name in enumerate(names):
        gw, gt, gtotal = gpu(eng, name)
        assert np.array_equal(w[i], gw) and np.array_equal(t[i], gt) and np.array_equal(w1[i], gw) and int(total[i]) == gtotal


# ---- 8. refusals
def test_refusals_raise_and_write_nothing(eng):
    import torch
    good = MC.record("turn_dead2")
    bad = good.copy()
    bad["board"][0, 1] = bad["board"][0, 0]
    batch = np.concatenate([good, bad])
    L = eng._lib
    win = np.full((2, ROWS, ROWS), 0xA5A5, np.uint16)
    tie = np.full((2, ROWS, ROWS), 0xA5A5, np.uint16)
    total = np.full(2, 0xA5A5A5A5, np.uint32)
    rc = L.mcq_exact_matrix(eng._ctx, batch.ctypes.data, 2, win.ctypes.data, tie.ctypes.data, total.ctypes.data)
    assert rc == _lib.MCQ_EINVAL and b"record 1: a table card is given twice" in L.mcq_last_error()
    assert (win == 0xA5A5).all() and (tie == 0xA5A5).all() and (total == 0xA5A5A5A5).all()
    d_win = torch.full((2, ROWS, ROWS), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        eng.exact_matrix_device(batch, d_win.data_ptr(), 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((d_win == 0x5A5A).all())
    for q in (_lib.pack_matrix_query(MC.CASES["flop_full"][0][:2]), _lib.pack_matrix_query(*MC.REFUSED_SHORT),
              np.zeros(0, _lib.MATRIX_QUERY_DTYPE), np.concatenate([good] * 257)):
        with pytest.raises(ValueError):
            eng.exact_matrix(q)
    with pytest.raises(ValueError):
        mh.get_equity_matrix(["AH", "KD"], engine=eng)
    win1, _, _ = eng.exact_matrix(good)                    # the same context goes on
    assert np.array_equal(win1[0], gpu(eng, "turn_dead2")[0])


# ---- 9. the reference's card strings
def test_get_equity_matrix_agrees_with_the_exact_seat_equities(eng):
    table, dead = ["AH", "KD", "7C"], ["2C", "2D"]
    win, tie, total = mh.get_equity_matrix(table, dead, engine=eng)
    assert win.shape == (ROWS, ROWS) and total == 43 * 42 // 2
    split, credited = mh.matrix_equity(win, tie, total), mh.matrix_equity(win, tie, total, ties="credited")
    for h, g in ((["QS", "JH"], ["QH", "JS"]), (["AS", "AC"], ["KS", "KC"]), (["7D", "6D"], ["AD", "QD"])):
        hi, gi = _lib.hand_index(*MC.C(*h)), _lib.hand_index(*MC.C(*g))
        shares = mh.get_seat_equities_exact([h, g], table, ghost_cards=dead, dealing="uniform")
        assert abs(split[hi, gi] - shares[0]) < 1e-12 and abs(split[gi, hi] - shares[1]) < 1e-12
        assert abs(split[hi, gi] + split[gi, hi] - 1.0) < 1e-12 and credited[hi, gi] >= split[hi, gi]
    assert np.isnan(split[_lib.hand_index(*MC.C("AH", "AS"))]).all()          # a table card: the hand meets nobody
    assert np.isnan(split[_lib.hand_index(*MC.C("2C", "3C"))]).all()          # a dead card
    plain = mh.get_equity_matrix(table, engine=eng)
    assert plain[2] == 990 and np.array_equal(plain[0], gpu(eng, "flop_full")[0])
