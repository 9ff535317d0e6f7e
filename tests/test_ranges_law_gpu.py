"""The law mcq_eval_batch_ranges deals, at 3 to 10 seats and on every street, against exact numbers from other code.

For every case of tests/ranges_law.py the reference is the all-in enumeration (Engine.exact_seats, uniform law), one
record per tuple of disjoint hands and one batch per case, weighted in Python integers with the tuples' weights
(ranges_law.expect_from_all_in).  That entry shares nothing with the ranges lane code beyond the evaluator, and its own
tests pin it to the host walk and the oracle.  The Monte-Carlo side is ONE record of 2^20 iterations; every seat's win,
tie and share and the whole trials per iteration (`passes`, which is what tells whole-trial rejection from any cheaper
scheme) are held to 5.5 sigma (tests/lawstats.py).  Fixed seeds: a failure is a finding about the law, never a reason
to widen the bound, drop a case or reseed.  The conditions under which a case tests anything -- acceptance at least 1/4,
expected counts of at least 100 or exactly 0, a tie and a win, the sequential law at least 10 sigma away -- are asserted
for every case by ranges_law.conditions."""
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from tests import lawstats as LS
from tests import ranges_law as RL
from tests import seats_expect as SE

pytestmark = pytest.mark.gpu
N = 1 << 20
SEED = 20261020


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w32(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 32)


def board_ids(case):
    return [RL.cid(c) for c in case["board"]]


def all_in_rows(eng, tl, board):
    """One exact_seats record per tuple, one batch: seat s of a row is seat s of the tuple."""
    p = len(tl[0][0])
    q = npa.pack_queries([hs[0] for hs, _ in tl], [board + [255] * (5 - len(board))] * len(tl), p, 1)
    ext = np.concatenate([_lib.pack_query_ext(1, known=[list(h) for h in hs[1:]]) for hs, _ in tl])
    rows = w32(eng.exact_seats(q, ext, law="uniform"))
    assert not rows[:, 1].any()
    return rows


def monte_carlo(eng, case, qid):
    p = len(case["supports"])
    tabs, st = RL.case_tables(case["supports"])
    seat_table = np.zeros((1, 10), np.uint32)
    seat_table[0, :p] = st
    q = _lib.pack_query_one([0, 0], board_ids(case), p, N)
    row = w32(eng.eval_batch_ranges(q, seat_table, tabs, SEED, first_query_id=qid))[0]
    SE.check_invariants(row, p)
    return row


@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4", "L5", "L6"])
def test_joint_law_against_the_all_in_enumeration(eng, name):
    """L1 river, 3 seats of 8 hands; L2 turn, 4 seats of 5 hands, seats 0 and 2 on the same table; L3 flop, 6 seats of 3
    hands; L4 flop, 10 seats of 2 hands; L5 flop, 6 seats of which three hold a known hand; L6 before the flop, 3 seats of
    2 hands -- its six tuples are six preflop all-in records of 1 370 754 completions each, whose time is printed."""
    case = RL.CASES[name]
    tl, a = RL.tuples(case["supports"], case["board"])
    t0 = time.perf_counter()
    rows = all_in_rows(eng, tl, board_ids(case))
    print("%s reference: %d all-in records in %.2f ms" % (name, len(tl), 1e3 * (time.perf_counter() - t0)))
    expect = RL.conditions(case["supports"], case["board"], tl, a, rows, N)
    row = monte_carlo(eng, case, 100 + int(name[1]))
    LS.check("%s, %d seats, %d tuples, a = %.4f" % (name, len(case["supports"]), len(tl), float(a)), RL.z_rows(row, expect, a, N))
    assert int(row[1]) > N


@pytest.mark.parametrize("name", ["L7", "L8"])
def test_one_full_width_seat_is_one_uniform_random_opponent(eng, name):
    """Every seat but one holds a known hand and that one holds weight 65535 on all 1326 hands (the table total at its
    maximum, 86 899 410): the law is that of ONE uniform random opponent, and the reference one record of
    Engine.exact_ext_seats with the uniform law, whose seats are the hero, the known hands, then the random seat."""
    case = RL.CASES[name]
    sup, board = case["supports"], board_ids(case)
    p = len(sup)
    known = [s for s in range(p) if len(sup[s]) == 1]
    rnd = [s for s in range(p) if len(sup[s]) != 1]
    assert len(rnd) == 1 and len(sup[rnd[0]]) == 1326 and set(sup[rnd[0]].values()) == {65535}
    order = known + rnd   # seat order[j] of the ranges record is seat j of the reference
    hands = [RL.hand(next(iter(sup[s]))) for s in known]
    q = npa.pack_queries([hands[0]], [board + [255] * (5 - len(board))], p, 1)
    ext = _lib.pack_query_ext(1, known=[list(h) for h in hands[1:]])
    ref = w32(eng.exact_ext_seats(q, ext, law="uniform"))
    _, a = RL.tuples(sup, case["board"])
    by_ref = RL.conditions([sup[s] for s in order], case["board"], [(tuple(range(p)), 1)], a, ref, N)
    expect = [None] * p
    for j, s in enumerate(order):
        expect[s] = by_ref[j]
    row = monte_carlo(eng, case, 100 + int(name[1]))
    LS.check("%s, %d seats, a = %.4f" % (name, p, float(a)), RL.z_rows(row, expect, a, N))
    assert int(row[1]) > N


def test_every_seat_a_known_hand(eng):
    """Six known hands on the turn: no trial is ever abandoned, the tallies are those of the single all-in record."""
    case = RL.CASES["H6"]
    tl, a = RL.tuples(case["supports"], case["board"])
    assert len(tl) == 1 and a == 1
    expect = RL.conditions(case["supports"], case["board"], tl, a, all_in_rows(eng, tl, board_ids(case)), N)
    row = monte_carlo(eng, case, 100)
    assert int(row[0]) == int(row[1]) == N                                          # passes == runs
    assert sum(int(x) for x in SE.seat_words(row)[:, 2]) == RL.UNIT * N              # sum_s share == MCQ_SHARE_UNIT * runs
    res = RL.z_rows(row, expect, a, N)
    assert len(res) == 18
    LS.check("H6, 6 known hands", res)
