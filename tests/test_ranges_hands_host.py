"""mcq_eval_batch_ranges_hands on the host: the lane code with the per-hand accumulator and the block tally of mcq_hands.hpp
(tests/hostsim_ranges_hands, walked in the kernel's block / round / wave order) against the recount of the deals that the
plain ranges host build hands back (tests/ranges_hands_expect.py), the flush bound of the table's uint32 words, and the law
per hand against the literal enumeration."""
import numpy as np
import pytest

from neuron_poker_amd import _lib
from tests import hostbuild
from tests import hostsim_ranges as HR
from tests import hostsim_ranges_hands as HH
from tests import lawstats as LS
from tests import ranges_hands_expect as X
from tests.ranges_law import cid, hand, hidx, joint_law, sequential_law, table, tuples

UNIT = 2520


@pytest.mark.parametrize("case", range(len(X.CASES)), ids=["%d cards %d seats %d runs" % c[:3] for c in X.CASES])
def test_host_build_is_the_recount(case):
    nb, p, runs, seats = X.CASES[case]
    row, per_seat = X.expect(case)
    q, st = X.record(case)
    for seat in (0, p - 1):
        got_row, got = HH.run(q, st, X.tables(), X.SEED, 0, seat)
        assert np.array_equal(got_row, row)                      # the seats row is hostsim_ranges's
        assert np.array_equal(got, per_seat[seat]), seat          # the rows are the recount, bit for bit
        X.check_sums(got_row, got, seat)
        # zero rows: hands of zero weight and hands on the table
        w = X.tables()[seats[seat]]
        on_table = {cid(c) for c in X.BOARD[:nb]}
        for b in range(52):
            for a in range(b):
                if w[X.hidx(a, b)] == 0 or a in on_table or b in on_table:
                    assert not got[X.hidx(a, b)].any(), (a, b)
        assert int(got[:, 0].sum()) == runs


def test_rows_do_not_depend_on_the_launch_shape():
    """One block or many, sixteen waves or one, other prices, a batch or single records: the same rows (contract 5)."""
    cases = [4, 6, 1, 13]   # 16384 runs at 2 seats, 2500 at 6, 17 at 3, 2500 at 3 with a known hand
    qs = np.concatenate([np.atleast_1d(X.record(c)[0]) for c in cases])
    st = np.stack([X.record(c)[1] for c in cases])
    want = [X.expect(c, qid=10 + i) for i, c in enumerate(cases)]
    for grid, waves, trials in ((1, 16, None), (7, 16, None), (3, 4, [1, 256, 3, 1]), (40, 1, None), (2, 5, [9, 1, 1, 200])):
        rows, hands = HH.run_batch(qs, st, X.tables(), X.SEED, 10, 0, grid=grid, waves=waves, trials=trials)
        for i, (row, per_seat) in enumerate(want):
            assert np.array_equal(rows[i], row), (grid, waves, i)
            assert np.array_equal(hands[i], per_seat[0]), (grid, waves, i)
    # a batch split in two with the matching first query id
    a = HH.run_batch(qs[:1], st[:1], X.tables(), X.SEED, 10, 0, grid=2)
    b = HH.run_batch(qs[1:], st[1:], X.tables(), X.SEED, 11, 0, grid=5)
    assert np.array_equal(a[1][0], want[0][1][0]) and all(np.array_equal(b[1][i], want[1 + i][1][0]) for i in range(3))


def test_one_hot_watched_seat():
    """Contract 6: a known hand's one row is the seat's whole row."""
    case = 9   # turn, seat 0 holds AH KH
    row, per_seat = X.expect(case)
    got_row, got = HH.run(*X.record(case), X.tables(), X.SEED, 0, 0)
    h = X.hidx(cid("AH"), cid("KH"))
    assert [int(x) for x in got[h]] == [int(row[0]), int(row[2]), int(row[3]), int(row[4])]
    assert not np.delete(got, h, axis=0).any()


def test_refusals_and_the_failure_marker():
    t = table({"ASAH": 1})
    q = X.query(5, 2, 10)
    for seat in (2, 9, 10):   # no such seat
        with pytest.raises(ValueError) as e:
            HH.run(q, [0, 0], X.tables(), 1, 0, seat)
        assert e.value.args[0] == -1
    with pytest.raises(ValueError) as e:   # a seat_table entry >= n_tables
        HH.run(q, [0, 4], X.tables(), 1, 0, 0)
    assert e.value.args[0] == -1
    with pytest.raises(ValueError) as e:   # two seats one-hot on the same hand: no accepted trial
        HH.run(X.query(5, 2, 1), [0, 0], t[None, :], 1, 0, 0)
    assert e.value.args[0] == HH.FAILED


# ------------------------------------------------------------------------------------------------------ the flush bound
def test_flush_bound():
    """The table's words are uint32 and a hand may take 2520 in every iteration (a one-hot seat that always wins).  The
    tally header is driven directly, no iteration dealt.  With the rule -- a flush after 64 rounds of 16384 -- the 64-bit
    row is exact at 64 x 16384 + 1 adds and at 105 rounds; without a flush the same adds at 105 rounds wrap the word (a word
    holds 104 rounds: 64 x 16384 + 1 adds of 2520 are 2.6e9 and do not reach 2^32 yet, so the case that CAN fail is the
    longer one)."""
    k = HH.constants()
    assert (k["table_words"], k["round_iters"], k["flush_rounds"], k["share_unit"]) == (1326 * 4, 16384, 64, UNIT)
    assert k["flush_rounds"] * k["round_iters"] * UNIT < 2 ** 32 <= 105 * k["round_iters"] * UNIT
    win = HH.increment(1)
    assert win & 0xFFFF == UNIT
    a, b = cid("AH"), cid("AS")
    n = 64 * 16384 + 1
    row, flushes, other = HH.drive(a, b, win, n, True)
    assert row == [n, n, 0, UNIT * n] and flushes == 1 and other == 0
    n = 105 * 16384
    assert UNIT * n >= 2 ** 32
    row, flushes, other = HH.drive(a, b, win, n, True)
    assert row == [n, n, 0, UNIT * n] and flushes == 1 and other == 0
    row, flushes, other = HH.drive(a, b, win, n, False)
    assert flushes == 0 and row[:3] == [n, n, 0] and row[3] == (UNIT * n) % 2 ** 32 != UNIT * n   # wrapped: the case can fail
    # ties: 2520 / k from the table, into the tie word
    row, _, other = HH.drive(0, 1, HH.increment(4), 1000, True)
    assert row == [1000, 0, 1000, 630 * 1000] and other == 0


def test_flush_in_the_middle_of_a_record_on_the_host():
    """One block of ONE wave: a round is one task, so 66 tasks are 66 rounds and the rule flushes in the middle of the
    record; the rows are those of sixteen waves, where nothing is flushed before the end."""
    runs = 66 * 1024 + 3
    q = X.query(5, 2, runs)
    want = HH.run(q, [3, 2], X.tables(), 5, 1, 0, grid=1, waves=16, flushes=True)
    got = HH.run(q, [3, 2], X.tables(), 5, 1, 0, grid=1, waves=1, flushes=True)
    assert want[2] == 0 and got[2] == 1
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    X.check_sums(got[0], got[1], 0)
    assert np.array_equal(got[0], HR.run(q, [3, 2], X.tables(), 5, 1))


def test_pieces_cover_every_task_once():
    """Whatever the grid: the blocks' pieces of a record are disjoint and cover its tasks."""
    g = np.random.default_rng(3)
    for _ in range(200):
        n_tasks, weight = int(g.integers(1, 70)), int(g.integers(1, 5000))
        pfx = int(g.integers(0, 10 ** 6))
        total = pfx + n_tasks * weight + int(g.integers(0, 10 ** 6))
        grid = int(g.integers(1, 300))
        seen = []
        for b in range(grid):
            first, end, rounds = HH.piece(pfx, weight, n_tasks, total * b // grid, total * (b + 1) // grid, 16)
            assert rounds == -(-(end - first) // 16)
            seen += list(range(first, end))
        assert seen == list(range(n_tasks))


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_sanitized_program(tmp_path, opt):
    """The tally header at the ends of its table, the flush bound and the pieces under AddressSanitizer and
    UndefinedBehaviorSanitizer."""
    lines = hostbuild.run_sanitized("hostsim_ranges_hands/hs_main.cpp", opt, tmp_path)
    assert lines[-1] == "ok: 7" and all(ln.endswith(": holds") for ln in lines[:-1]), lines


# ------------------------------------------------------------------------------------------------------ the law per hand
RIVER = ["2C", "7D", "9H", "JS", "KC"]
# the case of tests/test_ranges_host.py: overlapping cards on purpose; '9HAC' and 'KCQS' hold a table card: eff = 0
S0 = {"ASAH": 3, "ASKD": 5, "QDQH": 1, "TDTC": 7, "8C8D": 2, "9HAC": 6, "AHQD": 4, "5C6C": 1}
S1 = {"ASAD": 2, "AHKD": 7, "QDJD": 3, "TDTH": 1, "4C4D": 5, "KCQS": 4, "8C3D": 6, "ASQH": 2}
S2 = {"ASQC": 1, "4C5D": 3, "TD8D": 2, "6S6H": 7, "AHAD": 4, "3D3C": 5, "QHQS": 6}


def z_of(k, n, p):
    return (k / n - p) / max((p * (1.0 - p) / n) ** 0.5, 1.0 / n)


def test_law_per_hand_three_seats():
    """Watched seat 1 of (S0, S1, S2) on the river, 300 000 iterations: how often each hand is dealt against the marginal
    of the joint law, win and tie given the hand against the literal enumeration (on the river a deal decides the pot: the
    oracle's comparison of the three hands), 5.5 sigma.  The sequential law's marginal lies more than 10 sigma away for at
    least one hand: the test can tell the two apart."""
    from oracle import oracle as O
    supports, n, seat = (S0, S1, S2), 300000, 1
    tabs = np.stack([table(s) for s in supports])
    q = _lib.pack_query_one([0, 0], [cid(c) for c in RIVER], 3, n)
    row, got = HH.run(q, [0, 1, 2], tabs, 20261, 5, seat, grid=3)
    law = joint_law(supports, RIVER)
    board = [cid(c) for c in RIVER]
    marg, win, tie = {}, {}, {}
    for deal, pr in law.items():
        h = deal[seat]
        marg[h] = marg.get(h, 0.0) + pr
        keys = [list(x) + board for x in deal]
        best = [0]
        for s in range(1, 3):
            c = O.compare(keys[s], keys[best[0]])
            best = [s] if c > 0 else best + [s] if c == 0 else best
        if seat in best:
            d = win if len(best) == 1 else tie
            d[h] = d.get(h, 0.0) + pr
    assert len(marg) == 7   # 'KCQS' holds a table card
    res = []
    for h, pm in marg.items():
        r = [int(x) for x in got[hidx(h)]]
        res.append(("P(%s)" % (h,), r[0] / n, pm, z_of(r[0], n, pm)))
        assert r[0] > 1000
        for name, d, k in (("win", win, r[1]), ("tie", tie, r[2])):
            pc = d.get(h, 0.0) / pm
            res.append(("%s | %s" % (name, h), k / r[0], pc, z_of(k, r[0], pc)))
    LS.check("law per hand, seat 1 of three", res)
    assert sum(int(got[hidx(h), 0]) for h in marg) == n and int(got[:, 0].sum()) == n   # nothing outside the support
    X.check_sums(row, got, seat)
    # the wrong law that is cheapest to fall into: seat by seat from what is left
    tl, _ = tuples(supports, RIVER)
    seq = {}
    for (hs_, _w), (hs2, pr) in zip(tl, sequential_law(supports, RIVER)):
        assert hs_ == hs2
        seq[hs_[seat]] = seq.get(hs_[seat], 0.0) + float(pr)
    gaps = [abs(seq[h] - marg[h]) / (marg[h] * (1 - marg[h]) / n) ** 0.5 for h in marg]
    assert max(gaps) >= 10.0, gaps
    assert hand("AHKD") in marg
