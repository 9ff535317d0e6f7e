"""The launch plans without a GPU (csrc/mcq_plan.hpp through tests/hostsim_plan): what turns a batch into a grid, a block
size, a cut and a path.  The GPU tests build their batches around Python statements of that arithmetic; a statement that
drifted from the C++ would leave a GPU test passing on another path than the one it was written for, so here

  * mirror: over seeded sweeps the header == tests/ext_grid.py (small_plan, geometry), tests/exact_grid.py (plan_exact,
    plan_ext) and tests/test_eval_kernel_matrix.py (pick_split), with counters that show every branch was reached;
  * literals: values derived by hand at 256 compute units;
  * rows: the parts without a mirror (geometry's MCQ_LOAD_WAVES, working-wave, MCQ_GRID_CAP and cut arms, the small-query
    cut, mcq_exact_hero_plan, the ranges price) against tests/hostsim_plan/plan_rows.inc, rows recorded from the host
    layer's own text before it moved into the header; the same rows through a program under the host sanitizers."""
import random
from math import comb
from types import SimpleNamespace as NS

import numpy as np

import neuron_poker_amd as npa
from tests import exact_grid as XG
from tests import ext_grid as G
from tests import hostbuild
from tests import hostsim_plan as P
from tests import ranges_law as RL
from tests import test_eval_kernel_matrix as KM

N_CU = (8, 64, 256, 304)


def _query(n_board=0, n_players=2, runs=1):
    return npa.pack_queries([[50, 51]], [list(range(n_board)) + [255] * (5 - n_board)], n_players, runs)


def test_geometry_equals_the_mirror_of_the_extended_grid():
    rng = random.Random(20261020)
    few, per_cu, full, floor4 = 0, 0, 0, 0
    for n_cu in N_CU:
        for occ in (1, 2):
            top = 16 * n_cu * occ
            totals = set(range(1, 40)) | {n_cu * k + d for k in range(1, 18) for d in (-1, 0, 1)} | {top - 1, top, top + 1, 3 * top}
            totals |= {rng.randint(1, 2 * top) for _ in range(200)}
            for total in sorted(totals):
                grid, wpb = G.geometry(total, n_cu, occ)
                assert P.geometry(total, n_cu, occ) == (grid, 64 * wpb, 0, 0), (total, n_cu, occ)
                # the bulk kernel launches the same blocks when nothing is cut and no wave only loads
                assert P.geometry(total, n_cu, occ, bulk=True, split_max=0, load_waves=1) == (grid, 64 * wpb, 0, 0)
                few += grid < n_cu
                per_cu += grid == n_cu
                full += grid == n_cu * occ and occ == 2
                floor4 += -(-total // n_cu) < 4
    assert few > 100 and per_cu > 500 and full > 100 and floor4 > 300


def test_cut_equals_the_mirror_of_the_kernel_matrix():
    rng = random.Random(20261021)
    seen = [0] * 5
    by_total, by_most, by_max = 0, 0, 0
    for case in range(2000):
        n_cu, split_max = rng.choice(N_CU), rng.randint(0, 4)
        n = rng.choice((1, 1, 2, 3, 8, 40))
        runs = [rng.choice((1, 1000, 1024, 1025, 5000, 20000, 100000, 600000)) for _ in range(n)]
        q = npa.pack_queries([[0, 1]] * n, [[255] * 5] * n, 2, runs)
        total, most = int(KM.tasks(q).sum()), int(KM.tasks(q).max())
        want = KM.pick_split(q, n_cu, split_max)
        assert P.pick_split(total, most, n_cu, split_max) == want, (runs, n_cu, split_max)
        assert P.geometry(total, n_cu, 2, bulk=True, max_tasks=most, split_max=split_max)[2] == want
        seen[want] += 1
        if want < split_max:
            by_total += total << (want + 1) > 8 * n_cu
            by_most += most << (want + 1) > 512
        by_max += want == split_max
    assert min(seen) > 20 and by_total > 100 and by_most > 100 and by_max > 100, (seen, by_total, by_most, by_max)


def test_one_launch_plan_equals_the_mirror_of_the_extended_grid():
    assert P.ext_small_limits() == (G.SMALL_Q, G.SMALL_LISTS, G.SMALL_TASKS, G.SMALL_BLOCKS) == (8, 6, 64, 32)
    rng = random.Random(20261022)
    wpbs, refused, whole, cut = {4: 0, 8: 0, 16: 0}, 0, 0, 0
    for case in range(3000):
        n = rng.randint(1, 9)
        hi = rng.choice((1, 4, 5, 16, 17, 64, 65))
        recs = [NS(tasks=rng.randint(1, hi), lists=rng.choice((0, 1, 3, 6, 6, 7)) if case % 3 == 0 else rng.randint(0, 6)) for _ in range(n)]
        want = G.small_plan(recs)
        fits = P.ext_small_fits(n, max(max(r.lists for r in recs), 1), max(r.tasks for r in recs))
        assert fits == (want is not None), [(r.tasks, r.lists) for r in recs]
        if want is None:
            refused += 1
            continue
        wpb, blocks, first = P.ext_small_plan([r.tasks for r in recs])
        assert (wpb, [first[i + 1] - first[i] for i in range(n)], len(blocks)) == want
        assert first[0] == 0 and first[n] == len(blocks) <= G.SMALL_BLOCKS
        assert blocks == [(i, p, want[1][i], wpb) for i in range(n) for p in range(want[1][i])]
        wpbs[wpb] += 1
        whole += any(p == 1 for p in want[1])
        cut += any(p > 1 for p in want[1])
    assert min(wpbs.values()) > 50 and refused > 300 and whole > 300 and cut > 300, (wpbs, refused, whole, cut)


def test_exact_plans_equal_the_mirrors_of_the_exact_grid():
    sliced, capped, few = 0, 0, 0
    for n_cu in N_CU + (1, 2, 1000):
        for nb in (0, 3, 4, 5):
            for n_players in (1, 2, 3):
                grid, slices, units, _ = XG.plan_exact(NS(nb=nb, n_players=n_players), n_cu)
                n_boards, got_slices, row, got_grid = P.exact_plan(_query(nb, n_players), n_cu, row=9)
                assert (got_grid, got_slices, n_boards * got_slices, row) == (grid, slices, units, 9), (n_cu, nb, n_players)
                sliced += slices > 1
                capped += grid == n_cu
                few += grid < n_cu
    assert sliced >= 8 and capped >= 20 and few >= 20
    kinds, group_arms = [0, 0, 0], {"one": 0, "boards": 0, "share": 0}
    for n_cu in N_CU + (1, 2, 1000):
        for nb in (0, 3, 4, 5):
            for kind in (0, 1, 2):
                for L in range(43, 51):
                    if L > 50 - nb:
                        continue
                    grid, groups, n_boards = XG.plan_ext(NS(nb=nb, kind=kind, L=L), n_cu)
                    got = P.exact_ext_plan(_query(nb), kind, L, n_cu, ext=3, row=4, h1_off=60)
                    assert got == (grid, 3, n_boards, 4, grid, groups, 60), (n_cu, nb, kind, L)
                    assert n_boards == comb(L, 5 - nb)
                    kinds[kind] += 1
                    if kind == 2:
                        per = grid // groups
                        group_arms["one" if n_cu < groups else "boards" if per == n_boards else "share"] += 1
    assert min(kinds) > 100 and min(group_arms.values()) >= 7, (kinds, group_arms)


def test_values_derived_by_hand_at_256_compute_units():
    # two players, no table cards: C(50, 5) completions, sixteen per block and more than 256 blocks of them
    assert comb(50, 5) == 2118760
    assert P.exact_plan(_query(0, 2), 256) == (2118760, 1, 0, 256)
    # three players: the first opponent's loop is cut while completions x slices < 6 waves x 256 CUs x 4, at most in 64;
    # river: 1 x 64 units in blocks of six waves = 11 blocks; turn: 46 x 64 = 2944 units, 491 blocks, capped at the CUs
    assert P.exact_plan(_query(5, 3), 256) == (1, 64, 0, 11)
    assert P.exact_plan(_query(4, 3), 256) == (46, 64, 0, 256)
    # one block per CU: ceil(tasks / 256) working waves of the sixteen that load the tables (tests/test_long_queries_gpu.py)
    for tasks, waves in ((1008, 4), (1124, 5), (2016, 8)):
        grid, block, split, work = P.geometry(tasks, 256, 1, bulk=True, max_tasks=tasks)
        assert (block, split, work) == (1024, 0, waves) and grid == -(-tasks // waves)
    # eight queries of 64 tasks: 16 waves each block, 4 blocks each query, all 32 block words in use
    wpb, blocks, first = P.ext_small_plan([64] * 8)
    assert wpb == 16 and first == list(range(0, 33, 4)) and blocks[-1] == (7, 3, 4, 16)


def test_rows_recorded_before_the_plans_moved():
    rows = P.rows()
    assert {k: len(v) >= 12 for k, v in rows.items()} == dict.fromkeys(P.ROW_KINDS, True), {k: len(v) for k, v in rows.items()}
    for kind, mine in rows.items():
        for row in mine:
            assert P.row_holds(kind, row), (kind, row)
            assert not P.row_holds(kind, (row[0] + 1,) + row[1:]), (kind, row)     # (the checker does look at the results)
    # every arm of the parts that have no mirror
    geo = rows["PLAN_GEOMETRY"]
    assert any(r[10] == 0 and r[6] == 0 for r in geo) and any(r[10] == 0 and r[0] == r[6] for r in geo)   # unknown task count
    assert any(r[3] for r in geo) and any(r[9] and r[10] and not r[3] and r[8] > 1 for r in geo)         # working waves or none
    assert any(r[9] and r[8] not in (1, 16) for r in geo) and any(r[2] for r in geo)                     # MCQ_LOAD_WAVES, the cut
    assert any(r[10] and r[6] and r[0] == r[6] for r in geo) and any(not r[9] and r[1] == 1024 for r in geo)
    cut = rows["PLAN_SMALL_CUT"]
    assert {r[0] for r in cut} == {0, 1, 2, 3} and any(r[2] > 1 for r in cut) and any(r[1] < r[4] for r in cut)
    assert any(r[0] == r[5] < 3 for r in cut)                                                            # MCQ_SPLIT_MAX
    hero = [r for r in rows["PLAN_EXACT_EXT"] if r[4]]
    assert any(r[4] == 2 and r[0] == 0 and r[9] for r in hero) and any(r[4] == 2 and r[9] == 0 for r in hero)   # the refusals
    assert any(r[4] == 2 and r[0] and r[2] == r[9] * r[3] for r in hero)                                 # blocks <= completions a launch
    assert any(r[2] == r[1] * r[3] for r in hero) and any(r[3] > r[8] for r in hero) and any(r[4] == 1 for r in hero)
    price = rows["PLAN_PRICE"]
    assert {r[1] for r in price} == {0, 1, 2} and {1, 100, 256} <= {r[0] for r in price}
    assert any(r[1] == 0 and r[0] not in (1, 100, 256) for r in price) and {r[4] for r in price} == {0, 3, 4, 5}


def test_price_of_the_law_cases_and_of_tables_that_block():
    # the synthetic tables of the rows are what their description says (numpy's statement of hs_rows.hpp)
    idx = {(a, b): b * (b - 1) // 2 + a for b in range(52) for a in range(b)}
    i = np.arange(1326)
    assert (P.synthetic_table(0, 0, 0, 7) == 7).all() and not P.synthetic_table(4, 0, 0, 0).any()
    one = P.synthetic_table(1, 40, 12, 9)
    assert one[idx[12, 40]] == 9 and one.sum() == 9
    assert np.array_equal(P.synthetic_table(2, 7, 3, 5), np.where(i % 7 == 3, 1 + i % 5, 0))
    card = P.synthetic_table(3, 17, 0, 2)
    assert card.sum() == 2 * 51 and all(card[k] == 2 for (a, b), k in idx.items() if 17 in (a, b))
    # the first pass: per card the weight of the hands that hold it
    t = RL.table(RL.CASES["L1"]["supports"][0])
    wc = P.with_card(t)
    assert wc[52] == t.sum() and wc[:52].sum() == 2 * t.sum()
    assert all(wc[c] == sum(int(t[k]) for (a, b), k in idx.items() if c in (a, b)) for c in range(52))
    # recorded from the entry point's own loop before it moved (tests/ranges_law.py's tables)
    want = {"L1": 1, "L2": 3, "L3": 1, "L4": 2, "L5": 2, "L6": 1, "L7": 1, "L8": 2, "H6": 1}
    for name, case in RL.CASES.items():
        tables, seats = RL.case_tables(case["supports"])
        board = [RL.cid(c) for c in case["board"]]
        q = npa.pack_queries([[255, 255]], [board + [255] * (5 - len(board))], len(seats), 1000)
        assert P.ranges_price(tables, q, seats) == (want[name], 0, 0, 0), name
    # one-hot tables: the same hand at two seats collides always (1 / 0.01), at three seats the cap; disjoint hands never
    q = lambda n: npa.pack_queries([[255, 255]], [[255] * 5], n, 1000)   # noqa: E731
    aces, kings = RL.table({"ASAH": 1})[None], RL.table({"KSKH": 5})[None]
    assert P.ranges_price(aces, q(2), [0, 0]) == (100, 0, 0, 0)
    assert P.ranges_price(aces, q(3), [0, 0, 0]) == (256, 0, 0, 0)
    assert P.ranges_price(np.concatenate([aces, kings]), q(2), [0, 1]) == (1, 0, 0, 0)
    # refusals name the first seat at fault: a table that is not there, a table with nothing clear of the table cards
    assert P.ranges_price(aces, q(3), [0, 1, 2]) == (0, 1, 1, 1)
    flop = npa.pack_queries([[255, 255]], [[RL.cid("AS"), 0, 1, 255, 255]], 2, 1000)
    assert P.ranges_price(np.concatenate([kings, aces]), flop, [0, 1]) == (0, 2, 1, 1)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp walks the rows of plan_rows.inc, built with AddressSanitizer and UndefinedBehaviorSanitizer."""
    lines = hostbuild.run_sanitized("hostsim_plan/hs_main.cpp", "-O1", tmp_path)
    rows = P.rows()
    names = ("geometry", "small_cut", "exact", "exact_ext", "price")
    assert lines[:5] == ["%s: %d of %d rows" % (n, len(rows[k]), len(rows[k])) for n, k in zip(names, P.ROW_KINDS)], lines
    assert lines[5:] == ["ext_small: wpb 16, blocks 32, last 7 3 4 16"], lines
