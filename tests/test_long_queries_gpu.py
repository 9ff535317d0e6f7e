"""Long queries on the GPU: what only many tasks of ONE query per wave, or run counts near 2^32, execute.

Part B -- many tasks per wave.  WaveTallyWays keeps the nine tie_ways counters as 10-bit fields and must be flushed after
MCQ_WAYS_TALLY_TASKS = 63 tasks of one query; at the full grid a wave sees 63 tasks of one query only from about 2.6e8
iterations on, which no CPU reference reaches bit for bit.  MCQ_GRID_CAP=1 launches the shipped kernels
with ONE block, so a query of a million iterations is some 250 tasks per wave, and the oracle still follows.  The one
block has as many working waves as mcq_plan_geometry gives the launch: 4 for 1008 tasks, 5 for 1124, 8 for 2016 (host
entry, one query; csrc/mcq_plan.hpp, pinned without a GPU by tests/test_plan_host.py), 16 for the batch of twelve and for the device entry.  So 1 032 192 and 2 064 384 iterations are 252 =
4 x 63 tasks for every wave -- the flush falls on the wave's last task and the end-of-query flush finds a clean tally --
and 1 150 000 iterations are 224 or 225 tasks per wave: three flushes, then a tail of 35 or 36 tasks.

The saturating board: hero 2C 3D on KC KD KH KS AS.  The reference scores quads on the table by the two highest distinct
ranks of all seven cards, so every hand ties in every iteration: each iteration adds to exactly one field, k =
n_players, and a lane's field stands at exactly 16 x 63 = 1008 of its 1023 when the flush comes.  k = 4, 7, 10 are the
top fields of the three registers, k = 2, 5, 8 the bottom ones.  (The packing itself -- why 63 and not 64, what a field
holds after every task -- is pinned without a GPU by tests/test_tally_host.py on csrc/mcq_tally.hpp; here the shipped
kernels run into it.)

Part C -- run counts at the top of the 32-bit range at the full geometry: single tasks (windows) against the oracle, and
whole queries of 2^32 - 1 iterations against identities that need no oracle.

Expected rows are computed once per process (a module cache), up to sixteen host threads at a time."""
import contextlib
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import ext_ways_cases as XC
from tests import hot_boards as HB
from tests import seats_expect as SE
from tests import ways_expect as W
from tests.test_ways_gpu import FRONTS

pytestmark = pytest.mark.gpu

THREADS = 16
SEED = (1 << 45) | 0x2F6E2B1
BASE = (1 << 33) + 4001                  # query ids: above 2^32, so the parity mode's seed (seed + id) wraps as well
LAST_TASK, MID, TWICE = 63 * 16 * 1024, 1150000, 2 * 63 * 16 * 1024
CAP_RUNS = (LAST_TASK, MID, TWICE)
# "The flush falls on the wave's last task" needs the wave's share of the query to be a whole multiple of 63 tasks.  How
# many waves of the one block take work is mcq_plan_geometry's choice (csrc/mcq_plan.hpp: 4 and 8 today); 63 x 16 tasks and
# twice that split into whole multiples of 63 for every power of two up to the block's 16 waves, and for no other
# count: if mcq_plan_geometry ever picks one, these two run counts must follow it.
assert all((r // 1024) % (63 * w) == 0 and r % 1024 == 0 for r in (LAST_TASK, TWICE) for w in (1, 2, 4, 8, 16))
SAT_HERO, SAT_BOARD = ("2C", "3D"), ("KC", "KD", "KH", "KS", "AS")
# B2: the cases in which k varies, then quads on the table with hero above them and a wheel on the table, at 6 players
MIXED = [(tuple(h), tuple(b), n) for h, b, n in list(W.CASES) + [HB.SITUATIONS[8] + (6,), HB.SITUATIONS[16] + (6,)]]
assert MIXED[7][:2] == (("AH", "2D"), ("9C", "9D", "9H", "9S")) and MIXED[8][:2] == (("6C", "KD"), ("AD", "2C", "3H", "4S", "5D"))
MIXED_OTHER_FRONTS = (1, 3)              # ten players before the flop; quads on the turn table: also uniform law and parity mode
# B4 / B5: extended queries
EXT_CASES = [
    dict(name="saturating_known", hero=list(SAT_HERO), board=list(SAT_BOARD), n=6, known=[["4H", "5D"]]),
    dict(name="saturating_top50", hero=list(SAT_HERO), board=list(SAT_BOARD), n=4, opp=XC.top_classes(0.5)),
    XC.CASES[0],
    XC.CASES[1],
]
EXT_QID = BASE + 100


def sat_id(runs, n):
    """Query id of the saturating board at n players: the 1 150 000-run ones are BASE .. BASE + 8, in front of the mixed
    cases (BASE + 9 ..), so that the batch of B3 is made of rows the single-query tests expect under the same ids."""
    return BASE + {MID: 0, LAST_TASK: 32, TWICE: 64}[runs] + n - 2


def mixed_id(j):
    return BASE + 9 + j


# ------------------------------------------------------------------------------------------- expected rows (host)
_rows = {}
_trace_room = threading.Semaphore(6)     # a ten-player trace of 1 150 000 iterations and its scores are some 200 MB


def _compute(job):
    kind = job[0]
    if kind == "plain":                  # words 0..12 of a plain query: the oracle's tallies
        _, omode, hero, board, n, runs, qid = job
        return O.run_batch(omode, W.query(hero, board, n, runs), SEED, qid, threads=1)[0]
    if kind == "trace":                  # 22 words from the oracle's per-iteration trace
        _, omode, hero, board, n, runs, qid = job
        with _trace_room:
            return W.expected_row_fast(omode, list(hero), list(board), n, runs, SEED, qid, threads=1)
    if kind == "ext":                    # words 0..12 of an extended query: oracle.run_ex
        _, omode, c, runs, qid = job
        return XC.oracle_tallies(omode, EXT_CASES[c], runs, SEED, qid)
    if kind == "host_ways":              # the host lane build's general 22-word row of ext_ways_cases.CASES[i]
        _, i, replay, runs, qid = job
        return XC.hostsim_row(i, runs, replay, general=True, seed=SEED, qid=qid)
    if kind == "host_seats":             # the host lane build's 32-word row of ext_ways_cases.CASES[i]
        _, i, runs, qid = job
        return SE.host_row(i, runs, SEED, qid)
    raise AssertionError(job)


def rows_of(jobs):
    """The rows of `jobs`, missing ones computed side by side (the longest first)."""
    def cost(j):                         # (runs is the last but one entry of every job, n_players the fifth of a plain one)
        return j[-2] * (j[4] if j[0] in ("plain", "trace") else 6)
    missing = sorted((j for j in dict.fromkeys(jobs) if j not in _rows), key=cost, reverse=True)
    if any(j[0] == "host_ways" for j in missing):
        from tests import hostsim_ext_ways
        hostsim_ext_ways.lib()           # (built on first use: once, before the threads ask for it)
    if any(j[0] == "host_seats" for j in missing):
        from tests import hostsim_seats
        hostsim_seats.lib()
    if missing:
        O.lib()
        with ThreadPoolExecutor(min(THREADS, len(missing))) as pool:
            for j, r in zip(missing, pool.map(_compute, missing)):
                _rows[j] = np.asarray(r, np.uint64)
    return [_rows[j] for j in jobs]


def saturating_row(plain, n, runs):
    """22 words: the oracle's 13, checked against what the board guarantees, then tie_ways[n - 2] = runs."""
    plain = [int(x) for x in plain]
    assert plain[0] == runs and plain[2] == 0 and plain[3] == runs, plain
    assert plain[4 + 7] == runs and sum(plain[4:13]) == runs, plain          # four of a kind, every time
    row = np.zeros(22, np.uint64)
    row[:13] = plain
    row[13 + n - 2] = runs
    return row


# ------------------------------------------------------------------------------------------------------ GPU side
@contextlib.contextmanager
def engine(monkeypatch, cap, law="reference", times=False):
    """A fresh engine that reads MCQ_GRID_CAP=cap at creation (None: the switch unset)."""
    if cap is None:
        monkeypatch.delenv("MCQ_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("MCQ_GRID_CAP", str(cap))
    e = npa.Engine(0, kernel_times=times)
    try:
        e.set_dealing_law(law)
        yield e
    finally:
        e.close()


def w13(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 13)


def w22(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 22)


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def query(hero, board, n, runs):
    b = [npa.card_id(c) for c in board]
    return npa.pack_queries([[npa.card_id(c) for c in hero]], [b + [255] * (5 - len(b))], n, runs)


# ---- B1
@pytest.mark.parametrize("runs", CAP_RUNS)
@pytest.mark.parametrize("omode,mode,law", FRONTS)
def test_one_field_climbs_to_1008_between_flushes(monkeypatch, omode, mode, law, runs):
    """mcq_eval_kernel<*, false, true>, one block: every lane adds 16 to the field of k = n_players in every task."""
    players = range(2, 11) if runs != TWICE else (2, 10)
    plain = rows_of([("plain", omode, SAT_HERO, SAT_BOARD, n, runs, sat_id(runs, n)) for n in players])
    with engine(monkeypatch, 1, law) as eng:
        for n, p in zip(players, plain):
            exp = saturating_row(p, n, runs)
            q = query(SAT_HERO, SAT_BOARD, n, runs)
            got = w22(eng.eval_batch_ways(q, SEED, first_query_id=sat_id(runs, n), mode=mode))[0]
            credited = w13(eng.eval_batch(q, SEED, first_query_id=sat_id(runs, n), mode=mode))[0]
            assert np.array_equal(credited, exp[:13]), (n, credited, exp[:13])       # the plain WaveTally, 224+ tasks per wave
            assert np.array_equal(got, exp), (n, got, exp)


# ---- B2
@pytest.mark.parametrize("omode,mode,law", FRONTS)
def test_mixed_ties_across_mid_query_flushes(monkeypatch, omode, mode, law):
    """Several fields of a register grow at once; rows from the oracle's per-iteration trace."""
    idx = range(len(MIXED)) if omode == O.MODE_CTR else MIXED_OTHER_FRONTS
    exp = rows_of([("trace", omode) + MIXED[j] + (MID, mixed_id(j)) for j in idx])
    if omode == O.MODE_CTR:
        W.assert_cases_vary(exp)
    with engine(monkeypatch, 1, law) as eng:
        for j, e in zip(idx, exp):
            hero, board, n = MIXED[j]
            q = query(hero, board, n, MID)
            got = w22(eng.eval_batch_ways(q, SEED, first_query_id=mixed_id(j), mode=mode))[0]
            assert np.array_equal(got, e), (j, got, e)
            assert got[13:].sum() == got[3] and not got[13 + n - 1:].any()
            assert np.array_equal(w13(eng.eval_batch(q, SEED, first_query_id=mixed_id(j), mode=mode))[0], e[:13]), j


# ---- B3
def test_waves_cross_from_one_long_query_into_the_next(monkeypatch):
    """Twelve long queries in one call, sixteen waves: a wave's slice ends inside a query after several flushes and the
    next wave starts there; n_add and dirty start afresh with every query.  Host entry and device entry."""
    torch = pytest.importorskip("torch")
    jobs = [("plain", O.MODE_CTR, SAT_HERO, SAT_BOARD, n, MID, sat_id(MID, n)) for n in range(2, 11)]
    jobs += [("trace", O.MODE_CTR) + MIXED[j] + (MID, mixed_id(j)) for j in range(3)]
    rows = rows_of(jobs)
    exp = np.stack([saturating_row(rows[n - 2], n, MID) for n in range(2, 11)] + rows[9:])
    q = np.concatenate([query(SAT_HERO, SAT_BOARD, n, MID) for n in range(2, 11)] + [query(*MIXED[j], MID) for j in range(3)])
    assert sat_id(MID, 10) + 1 == mixed_id(0)
    with engine(monkeypatch, 1) as eng:
        got = w22(eng.eval_batch_ways(q, SEED, first_query_id=BASE))
        assert np.array_equal(got, exp), (got, exp)
        assert np.array_equal(w13(eng.eval_batch(q, SEED, first_query_id=BASE)), exp[:, :13])
        # the device entry: the geometry of a launch whose task count the host does not know
        dq = torch.from_numpy(np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16).copy()).cuda()
        out = torch.full((len(q), 22), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.eval_batch_device_ways(dq.data_ptr(), len(q), SEED, out.data_ptr(), first_query_id=BASE,
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dev = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(dev, exp), (dev, exp)


# ---- B4 / B5
def ext_expected(c, replay):
    """22 words of EXT_CASES[c] under id EXT_QID + c: the oracle's 13, then the analytic field (saturating board) or the
    host lane build's general row."""
    omode = O.MODE_MT if replay else O.MODE_CTR
    if c < 2:
        (plain,) = rows_of([("ext", omode, c, MID, EXT_QID + c)])
        p = [int(x) for x in plain]
        assert p[0] == MID and p[2] == 0 and p[3] == MID and p[4 + 7] == MID, p
        row = np.zeros(22, np.uint64)
        row[:13] = plain
        row[13 + EXT_CASES[c]["n"] - 2] = MID
        return row
    plain, host = rows_of([("ext", omode, c, MID, EXT_QID + c), ("host_ways", c - 2, replay, MID, EXT_QID + c)])
    assert np.array_equal(host[:13], plain), (c, host, plain)
    return host


def prefetch_ext(seats):
    jobs = [("ext", m, c, MID, EXT_QID + c) for c in range(4) for m in ((O.MODE_CTR,) if seats else (O.MODE_CTR, O.MODE_MT))]
    jobs += [("host_ways", c - 2, r, MID, EXT_QID + c) for c in (2, 3) for r in ((False,) if seats else (False, True))]
    if seats:
        jobs += [("host_seats", c - 2, MID, EXT_QID + c) for c in (2, 3)]
    rows_of(jobs)


@pytest.mark.parametrize("mode", [npa.MODE_PHILOX, npa.MODE_REPLAY_MT19937], ids=["ctr", "replay"])
def test_extended_kernel_flushes_mid_query(monkeypatch, mode):
    """mcq_eval_ext_kernel<*, MCQ_ROW_WAYS>: the second flush site."""
    prefetch_ext(False)
    with engine(monkeypatch, 1) as eng:
        for c, case in enumerate(EXT_CASES):
            exp = ext_expected(c, mode == npa.MODE_REPLAY_MT19937)
            q, ext = XC.records(case, MID)
            got = w22(eng.eval_batch_ext_ways(q, ext, SEED, first_query_id=EXT_QID + c, mode=mode))[0]
            assert np.array_equal(got, exp), (case["name"], got, exp)
            assert got[13:].sum() == got[3]
            assert np.array_equal(w13(eng.eval_batch_ext(q, ext, SEED, first_query_id=EXT_QID + c, mode=mode))[0], got[:13])


def test_per_seat_rows_carried_across_many_tasks(monkeypatch):
    """WaveTallySeats: a lane's 64-bit word of the row, added to over some 225 tasks of one query."""
    prefetch_ext(True)
    with engine(monkeypatch, 1) as eng:
        for c, case in enumerate(EXT_CASES):
            n = case["n"]
            q, ext = XC.records(case, MID)
            got = w32(eng.eval_batch_ext_seats(q, ext, SEED, first_query_id=EXT_QID + c))[0]
            SE.check_invariants(got, n)
            ways = ext_expected(c, False)
            assert np.array_equal(w22(eng.eval_batch_ext_ways(q, ext, SEED, first_query_id=EXT_QID + c))[0], ways)
            assert [int(x) for x in got[:4]] == [int(x) for x in ways[:4]], (case["name"], got, ways)
            assert int(got[4]) == SE.hero_share_from_ways(ways), (case["name"], got, ways)
            seats = SE.seat_words(got)
            if c < 2:
                for s in range(n):
                    assert [int(x) for x in seats[s]] == [0, MID, SE.UNIT // n * MID], (case["name"], s, seats)
            else:
                (host,) = rows_of([("host_seats", c - 2, MID, EXT_QID + c)])
                assert np.array_equal(got, host), (case["name"], got, host)


# ---- B6
def test_the_cap_changes_nothing_but_the_number_of_blocks(monkeypatch):
    runs = 9000
    q = np.concatenate([query(h, b, n, runs) for h, b, n in W.CASES])
    ext = npa.pack_query_ext(len(q))
    seen = []
    for cap in (None, 1, 3):
        with engine(monkeypatch, cap) as eng:
            seen.append((w13(eng.eval_batch(q, W.SEED, first_query_id=W.QID)).copy(),
                         w22(eng.eval_batch_ways(q, W.SEED, first_query_id=W.QID)).copy(),
                         w22(eng.eval_batch_ext_ways(q, ext, W.SEED, first_query_id=W.QID)).copy()))
    raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)
    assert np.array_equal(seen[0][0], O.run_batch(O.MODE_CTR, raw, W.SEED, W.QID, threads=len(q)))
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert np.array_equal(a, b), (a, b)


# ---- C1
TOP = 2 ** 32 - 1
WINDOW_SHAPES = [(("AH", "KH"), ("2C", "7D", "9S", "JH", "3C"), 2), (("7C", "2D"), (), 6), (("QS", "QD"), ("2C", "7D", "9S", "JH"), 10)]
WINDOW_QID = (1 << 40) + 5


@pytest.mark.parametrize("omode,law", [(O.MODE_CTR, "reference"), (O.MODE_CTR_UNIFORM, "uniform")], ids=["reference", "uniform"])
@pytest.mark.parametrize("runs", [TOP, 2 ** 32 - 1024, 2 ** 31 + 1])
def test_single_tasks_of_a_query_near_2_to_the_32(monkeypatch, omode, law, runs):
    """part = (p, T) with T = the query's task count is exactly task p: 1024 iterations of streams 64 p .. 64 p + 63,
    iterations 1024 p ...  The oracle runs just those (mcqo_run_range)."""
    T = (runs + 1023) // 1024
    q = np.concatenate([query(h, b, n, runs) for h, b, n in WINDOW_SHAPES])
    raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1, 16)
    with engine(monkeypatch, None, law) as eng:
        for p in sorted({0, 1, 2 ** 21 - 1, 2 ** 21, T - 2, T - 1}):
            exp = O.run_batch_part(omode, raw, SEED, WINDOW_QID, p, T)
            want_runs = min(1024, runs - 1024 * p)
            assert (exp[:, 0] == want_runs).all() and exp[:, 2:4].sum() > 0, (p, exp)
            for i in range(len(q)):     # one query, one task, one wave
                got = w13(eng.eval_batch(q[i:i + 1], SEED, first_query_id=WINDOW_QID + i, part=(p, T)))[0]
                assert np.array_equal(got, exp[i]), (runs, p, i, got, exp[i])
            assert np.array_equal(w13(eng.eval_batch(q, SEED, first_query_id=WINDOW_QID, part=(p, T))), exp), (runs, p)
        if runs == TOP:
            last = w13(eng.eval_batch(q, SEED, first_query_id=WINDOW_QID, part=(T - 1, T)))
            assert (last[:, 0] == 1023).all(), last


# ---- C2
def test_whole_query_of_2_to_the_32_minus_1_runs_saturating_board(monkeypatch):
    """Ten players, every iteration a ten-way tie: each counter of the row is known without an oracle."""
    with engine(monkeypatch, None, times=True) as eng:
        got = [int(x) for x in w22(eng.eval_batch_ways(query(SAT_HERO, SAT_BOARD, 10, TOP), SEED, first_query_id=BASE))[0]]
        print("2^32-1 runs, saturating board, 10 players, eval_batch_ways: kernel %.1f ms" % eng.last_kernel_ms)
    exp = [0] * 22
    exp[0], exp[1], exp[3], exp[4 + 7], exp[13 + 8] = TOP, 9 * TOP, TOP, TOP, TOP
    assert got == exp, (got, exp)


def test_whole_extended_query_of_2_to_the_32_minus_1_runs(monkeypatch):
    """Six players, one of them a known hand, on the saturating board: split-pot and per-seat rows."""
    case = EXT_CASES[0]
    small = XC.oracle_tallies(O.MODE_CTR, case, 4096, SEED, BASE)
    assert int(small[1]) == 4 * 4096     # one attempt per random opponent: nothing is ever re-drawn here
    q, ext = XC.records(case, TOP)
    with engine(monkeypatch, None, times=True) as eng:
        ways = [int(x) for x in w22(eng.eval_batch_ext_ways(q, ext, SEED, first_query_id=BASE))[0]]
        print("2^32-1 runs, saturating board, 6 players, eval_batch_ext_ways: kernel %.1f ms" % eng.last_kernel_ms)
        seats = w32(eng.eval_batch_ext_seats(q, ext, SEED, first_query_id=BASE))[0]
        print("2^32-1 runs, saturating board, 6 players, eval_batch_ext_seats: kernel %.1f ms" % eng.last_kernel_ms)
    exp = [0] * 22
    exp[0], exp[1], exp[3], exp[4 + 7], exp[13 + 4] = TOP, 4 * TOP, TOP, TOP, TOP
    assert ways == exp, (ways, exp)
    SE.check_invariants(seats, 6)
    assert [int(x) for x in seats[:2]] == [TOP, 4 * TOP]
    s = SE.seat_words(seats)
    assert sum(int(x[2]) for x in s) == SE.UNIT * TOP
    for k in range(10):
        assert [int(x) for x in s[k]] == ([0, TOP, SE.UNIT // 6 * TOP] if k < 6 else [0, 0, 0]), (k, s)


@pytest.mark.parametrize("law", ["reference", "uniform"])
def test_whole_heads_up_query_of_2_to_the_32_minus_1_runs(monkeypatch, law):
    hero, board = ("AH", "KH"), ("2C", "7D", "9S", "JH")
    q = query(hero, board, 2, TOP)
    with engine(monkeypatch, None, law, times=True) as eng:
        row = w13(eng.eval_batch(q, SEED, first_query_id=BASE))[0]
        print("2^32-1 runs, heads-up turn, %s law, eval_batch: kernel %.1f ms" % (law, eng.last_kernel_ms))
        parts = np.stack([w13(eng.eval_batch(q, SEED, first_query_id=BASE, part=(p, 8)))[0] for p in range(8)])
        ways = w22(eng.eval_batch_ways(q, SEED, first_query_id=BASE))[0]
        print("2^32-1 runs, heads-up turn, %s law, eval_batch_ways: kernel %.1f ms" % (law, eng.last_kernel_ms))
    r = [int(x) for x in row]
    assert r[0] == TOP and r[1] == TOP and sum(r[4:13]) == r[2] + r[3], r
    assert np.array_equal(parts.sum(axis=0, dtype=np.uint64), row), (parts, row)
    assert np.array_equal(ways[:13], row) and int(ways[13]) == r[3] and not ways[14:].any(), (ways, row)
    win, tie, _ = O.exact(list(hero), list(board), 2, law == "uniform")     # the CPU tree walk
    p = win + tie
    sigma = (p * (1 - p) / TOP) ** 0.5
    got = (r[2] + r[3]) / TOP
    print("equity %.7f, exact %.7f, %.2f sigma" % (got, p, (got - p) / sigma))
    assert abs(got - p) <= 5 * sigma, (got, p, sigma)
