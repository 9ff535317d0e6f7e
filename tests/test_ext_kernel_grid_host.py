"""The extended-query grid (tests/ext_grid.py) without a GPU: the expected rows that tests/test_ext_kernel_grid_gpu.py
compares the kernels with are pinned here, independently of the lane code that produced them.

  * words 0..12 of EVERY grid record, from the host lane build in the form the kernels pick (and, for the fast form's
    records, in the general form too), equal the oracle's tallies (oracle.run_ex, the independent C restatement);
  * words 13..21 equal a recount of the hands the host build dealt, with the oracle's comparison, for one record of every
    kind under every stream rule the kind has;
  * the per-seat rows of every record: hero's columns are the split-pot row's, a pot is handed out whole in every
    iteration, and the seats are recounted from the dealt hands on the same subset;
  * the grid's own assertions (no cell left out, every run count, both stream rules, every record dealable), and the
    verdicts of the mirrors of the host layer's path choice and of the kernels' list placement for the GPU file's batches
    at the MI355X's 256 compute units."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ext_grid as G
from tests import ext_ways_cases as XC
from tests import hostsim_ext_ways as H
from tests import hostsim_seats as HS
from tests import hostsim_ways as HW
from tests import seats_expect as SE


def indexed(kind):
    return [(j, r) for j, r in enumerate(G.grid()) if r.kind == kind]


def test_grid_leaves_nothing_out():
    recs = G.grid()
    G.assert_grid(recs)
    assert G.SEED >= 1 << 40 and G.FQ != 0
    assert len({r.cell for r in recs}) == len(G.CELLS) == 36 * 7 + 20
    # ranges: 40 classes at least
    for r in recs:
        for h in [r.oracle_args["hero"], r.oracle_args["opp"]] + r.oracle_args["known"]:
            assert h is None or len(h) == 2 or len(h) >= 40, r


@pytest.mark.parametrize("kind", G.KINDS)
def test_words_0_12_are_the_oracles(kind):
    """Every record of the kind can be dealt (the host build raises where it cannot: the share of such records is zero),
    and the host build's words 0..12 are the oracle's tallies."""
    for j, r in indexed(kind):
        row = G.ways_row(r, G.FQ + j)
        a = r.oracle_args
        want = O.run_ex(O.MODE_CTR, a["hero"], a["board"], r.players, r.runs, G.SEED, G.FQ + j, ghost=a["ghost"],
                        opp_range=a["opp"], known=a["known"])["tallies"].astype(np.uint64)
        assert np.array_equal(row[:13], want), (j, r)
        assert int(row[0]) == r.runs and int(row[13:22].sum()) == int(row[3]) and not row[13 + r.players - 1:22].any(), (j, r)
        if r.fast:
            assert np.array_equal(H.run(False, r.q, r.ext, G.SEED, G.FQ + j, general=True), row), (j, r)


def test_empty_record_is_the_plain_path():
    for j, r in indexed("K0"):
        assert np.array_equal(G.ways_row(r, G.FQ + j), HW.run(O.MODE_CTR, r.q, G.SEED, G.FQ + j)), (j, r)


def recount_subset():
    """One record per kind and stream rule: the cheapest (runs x players) that has more than one stream."""
    best = {}
    for j, r in enumerate(G.grid()):
        k = (r.kind, r.s_iters)
        if r.runs > r.s_iters and (k not in best or r.runs * r.players < best[k][1].runs * best[k][1].players):
            best[k] = (j, r)
    assert set(best) == {(k, 16) for k in G.KINDS} | {(k, 2) for k in ("K1", "K4", "K5", "K6", "K7")}
    return sorted(best.values(), key=lambda x: x[0])


def test_words_13_21_and_the_seats_are_a_recount_of_the_dealt_hands():
    for j, r in recount_subset():
        row, hands = H.run(False, r.q, r.ext, G.SEED, G.FQ + j, hands=True)
        assert (hands != 255).all() and np.array_equal(row, G.ways_row(r, G.FQ + j))
        ways, win, tie = XC.recount(hands, r.players)
        assert np.array_equal(row[13:22], ways) and (int(row[2]), int(row[3])) == (win, tie), (j, r)
        srow, shands = HS.run(r.q, r.ext, G.SEED, G.FQ + j, hands=True)
        assert np.array_equal(shands, hands) and np.array_equal(srow, G.seats_row(r, G.FQ + j))
        assert np.array_equal(SE.seat_words(srow), SE.recount(hands, r.players)), (j, r)


def test_seats_rows_follow_from_the_ways_rows():
    for j, r in enumerate(G.grid()):
        seats, ways = G.seats_row(r, G.FQ + j), G.ways_row(r, G.FQ + j)
        assert [int(x) for x in seats[:4]] == [int(x) for x in ways[:4]], (j, r)
        assert int(seats[4]) == SE.hero_share_from_ways(ways), (j, r)
        SE.check_invariants(seats, r.players)


def test_one_launch_mirror_gives_the_intended_cuts():
    for name, (recs, _, want) in G.small_batches().items():
        plan = G.small_plan(recs)
        assert plan is not None and (plan[0], plan[2]) == want, (name, plan)
        assert 1 <= len(recs) <= 8
    b = G.small_batches()
    assert {len(recs) for recs, _, _ in b.values()} >= {1, 2, 3, 5, 6, 7, 8}
    assert G.small_plan(b["wpb4_two_parts"][0])[1] == [2] * 8
    recs = b["one_64_task_query_among_one_task_queries"][0]
    wpb, parts, _ = G.small_plan(recs)
    assert any(p == 1 and r.tasks < wpb for p, r in zip(parts, recs)) and any(p > 1 for p in parts)
    assert {r.s_iters for r in b["streams_of_16"][0]} == {16} and any(r.lists for r in b["streams_of_16"][0])
    for name in ("wpb4_two_parts", "wpb8", "wpb16_32_blocks"):     # the fast form and the general form, some lists
        assert {r.fast for r in b[name][0]} == {False, True} and all(r.lists for r in b[name][0])
    for name, (recs, _, small) in G.fence_batches().items():
        assert (G.small_plan(recs) is not None) == small, name


def test_one_launch_header_gives_the_intended_cuts():
    """The same expectations against the host layer's own plan (csrc/mcq_plan.hpp through tests/hostsim_plan)."""
    from tests import hostsim_plan as P
    fits = lambda recs: P.ext_small_fits(len(recs), max(max(r.lists for r in recs), 1), max(r.tasks for r in recs))   # noqa: E731
    for name, (recs, _, want) in G.small_batches().items():
        assert fits(recs), name
        wpb, blocks, first = P.ext_small_plan([r.tasks for r in recs])
        assert (wpb, len(blocks)) == want, (name, wpb, len(blocks))
        assert [first[i + 1] - first[i] for i in range(len(recs))] == G.small_plan(recs)[1], name
    for name, (recs, _, small) in G.fence_batches().items():
        assert fits(recs) == small, name


def test_list_placement_mirror_gives_the_intended_branches():
    """At 256 compute units, one or two resident blocks per CU (the GPU file asserts the same at the device's count)."""
    verdicts = {name: G.placement_verdicts(recs, 256)[0] for name, (recs, _) in G.placement_batches().items()}
    assert verdicts["staged"] == [{"staged"}] * 2
    assert verdicts["no_block_stages"] == [{"entries"}] * 2
    assert verdicts["refused_by_entries"] == [{"entries"}] * 2
    assert verdicts["refusing_beside_staging"] == [{"entries", "staged"}] * 2
    b = G.placement_batches()
    assert 9 <= len(b["staged"][0]) <= 14
    for r in b["no_block_stages"][0]:     # eight lists of 168 classes at least: more entries than a block's LDS takes
        assert r.lists >= 8 and sum(H.list_len(r.q, r.ext, li) for li in range(r.lists)) >= 19000
    assert all(r.kind == "K1" and r.fast and r.tasks == 1 for r in b["refused_by_entries"][0])
    mixed = b["refusing_beside_staging"][0]
    assert all(r.lists >= 8 for r in mixed[:len(mixed) // 3]) and all(r.lists == 1 for r in mixed[len(mixed) // 3:])


def test_every_batch_of_the_gpu_file_can_be_dealt():
    """... outside the grid's canonical order too (a query's streams depend on its query id)."""
    for recs, fq, _ in list(G.small_batches().values()) + list(G.fence_batches().values()):
        G.expect(recs, fq, seats=False)
    for name, (recs, fq) in G.placement_batches().items():
        G.expect(recs, fq)
    recs, fq = G.shuffled()
    G.expect(recs, fq)
