"""The paired count of the dealing in epochs (mcq_hole_count2 and the biased registers of mcq_draw_epoch), without a GPU.

tests/hostsim_paired builds the lane code for the host with the switch (MCQ_COUNT_PAIRED's place in the template list) named
by the caller, so paired and unpaired text run side by side.

* The primitive against the direct count, exhaustively: every p in 0..49 against every pair of bytes a plain and a biased
  register can hold -- a coordinate 0..49 (t == p and t == p + 1 among them), a free slot moved down by 0..13 scans -- in
  every byte lane, and every fill level of the biased register (one to four holes) beside a full plain one.
* Positions against list.pop for 1 to 9 opponents x 0 to 5 table cards to come, by the plan of exactly those draws and by
  the plan of five table cards stopped early, every rule: the boundary rows of tests/test_epoch_dealing_host.py and 100 000
  random rows per shape; paired and unpaired equal word for word.
* Tallies of the 31 forms, both accumulators, both laws: against the oracle's CTR mode and against the unpaired text.
* Parity mode's straight forms against the oracle's MT19937 mode.
* The same lane code in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hostbuild
from tests import hostsim_join
from tests import hostsim_paired as P
from tests import test_epoch_dealing_host as T   # its rows, shapes and queries; nothing of it is collected from here

N_RANDOM = 100000


def splat(x):
    return (np.asarray(x, np.uint32) * np.uint32(0x01010101)).astype(np.uint32)


def test_the_switch_ships_on_or_off():
    assert P.shipped_switch() in (0, 1)


# -------------------------------------------------------------------------------------------------------- primitive
def byte_values(biased):
    """every byte a register can hold: a coordinate 0..49, a free slot moved down by 0..13 scans; -> (stored, coordinate or
    -1 for a free slot)"""
    stored = [t + (0x40 if biased else 0) for t in range(50)] + [0x7F - s for s in range(14)]
    return np.array(stored, np.uint32), np.array(list(range(50)) + [-1] * 14)


def test_count2_equals_the_direct_count_on_every_byte_pair():
    s0, t0 = byte_values(False)
    s1, t1 = byte_values(True)
    assert s1.max() <= 0x7F and s0.max() <= 0x7F
    p, a, b, lane = (v.ravel() for v in np.meshgrid(np.arange(50), np.arange(64), np.arange(64), np.arange(4), indexing="ij"))
    sh = (8 * lane).astype(np.uint32)
    keep = ~(np.uint32(0xFF) << sh)
    for filler0, filler1 in ((0x7F7F7F7F, 0x7F7F7F7F), (0x7F7F7F7F - 13 * 0x01010101, 0x7F7F7F7F - 13 * 0x01010101)):
        h0 = (np.uint32(filler0) & keep) | (s0[a] << sh)
        h1b = (np.uint32(filler1) & keep) | (s1[b] << sh)
        got, single = P.count2(splat(p | 0x80), h0, h1b)
        want = ((t0[a] >= 0) & (t0[a] <= p)).astype(np.uint32) + ((t1[b] >= 0) & (t1[b] <= p)).astype(np.uint32)
        assert len(p) == 50 * 64 * 64 * 4
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
        assert np.array_equal(single, want)
    # t == p and t == p + 1 in both registers at once
    for p0 in range(50):
        for d0 in (0, 1):
            for d1 in (0, 1):
                ta, tb = min(p0 + d0, 49), min(p0 + d1, 49)
                got, _ = P.count2(splat([p0 | 0x80]), splat([ta]), (splat([tb]) + np.uint32(P.BIAS)).astype(np.uint32))
                assert got[0] == 4 * int(ta <= p0) + 4 * int(tb <= p0), (p0, ta, tb, got)


def test_count2_at_every_fill_level_of_the_biased_register():
    """a full plain register beside a biased one with one to four holes, its free slots where the scans they have seen leave
    them (0..13 scans); random coordinates and every p"""
    rng = np.random.RandomState(4040)
    n = 20000
    for fill in (1, 2, 3, 4):
        for scans in range(14):
            p = rng.randint(0, 50, n)
            c0 = rng.randint(0, 50, (n, 4))
            c1 = rng.randint(0, 50, (n, 4))
            c0[: n // 4, 0] = p[: n // 4]                                       # t == p
            c1[n // 4: n // 2, 0] = np.minimum(p[n // 4: n // 2] + 1, 49)       # t == p + 1
            h0 = sum((c0[:, i].astype(np.uint32) << np.uint32(8 * i)) for i in range(4))
            b1 = np.where(np.arange(4)[None, :] < fill, c1 + 0x40, 0x7F - scans)
            h1b = sum((b1[:, i].astype(np.uint32) << np.uint32(8 * i)) for i in range(4))
            got, single = P.count2(splat(p | 0x80), h0, h1b)
            want = (c0 <= p[:, None]).sum(1) + (c1[:, :fill] <= p[:, None]).sum(1)
            assert np.array_equal(got, want.astype(np.uint32)), (fill, scans)
            assert np.array_equal(single, got)


# ------------------------------------------------------------------------------------------------------------ plans
def test_the_plans_pair_what_the_model_says():
    assert P.plan(15, 3)["cost"] == 143 and P.plan(15, 3)["cost_paired"] == 136
    assert P.plan(15, 3)["regs"][:3] == [0, 2, 0]          # {8, 12, 13}: register 1 is biased by its first scan
    assert P.plan(23, 3)["cost"] == 308 and P.plan(23, 3)["cost_paired"] == 286
    assert P.plan(23, 3)["regs"][:4] == [0, 2, 0, 2]       # {8, 16, 20}: two full pairs
    assert P.plan(15, 1)["regs"][:4] == [0, 2, 0, 1]       # {8}: the last epoch ends with six holes, biased by the pair draw
    seen = set()
    for n in range(2, 24):
        for rule in P.RULES:
            pl = P.plan(n, rule)
            assert pl["cost_paired"] <= pl["cost"]
            r = 0
            for holes in pl["holes"]:
                regs = (holes + 3) // 4
                counted = holes // 4 + (1 if holes % 4 >= 2 else 0)
                for i in range(regs):
                    want = 0 if (i % 2 == 0 or i >= counted) else (1 if holes == 4 * i + 2 else 2)
                    assert pl["regs"][r + i] == want, (n, rule, pl)
                    seen.add((want, min(holes - 4 * i, 4)))
                r += regs
    assert {(2, 4), (2, 3), (1, 2)} <= seen, seen          # a biased register full, partly filled, and closed behind its pair


# -------------------------------------------------------------------------------------------------------- positions
@pytest.mark.parametrize("rule", P.RULES)
def test_pattern_rows_equal_list_pop_and_the_unpaired_text(rule):
    for nopp, ndeal in T.SHAPES:
        n, deck_len = 2 * nopp + ndeal, 45 + ndeal
        d = T.pattern_rows(n, deck_len)
        want = T.list_pop_rows(d, deck_len)
        for n_plan in T.shape_plans(nopp, ndeal):
            got = P.positions(n_plan, rule, d, paired=True)
            bad = np.flatnonzero((got != want).any(1))
            assert len(bad) == 0, ((nopp, ndeal), n_plan, d[bad[0]], got[bad[0]], want[bad[0]])
            assert np.array_equal(got, P.positions(n_plan, rule, d, paired=False)), ((nopp, ndeal), n_plan)


def test_random_rows_equal_list_pop_and_the_unpaired_text():
    """100 000 random rows per shape, the expected positions worked out once per number of table cards (see
    tests/test_epoch_dealing_host.py)"""
    rng = np.random.RandomState(20920)
    for ndeal in range(0, 6):
        deck_len, n_max = 45 + ndeal, 18 + ndeal
        d_all = (rng.randint(0, 1 << 30, size=(N_RANDOM, n_max)) % (deck_len - np.arange(n_max))).astype(np.uint8)
        want_all = T.list_pop_numpy(d_all, deck_len)
        assert np.array_equal(want_all[:300], T.list_pop_rows(d_all[:300], deck_len))
        for nopp in range(1, 10):
            n = 2 * nopp + ndeal
            d, want = np.ascontiguousarray(d_all[:, :n]), want_all[:, :n]
            for rule in P.RULES:
                for n_plan in T.shape_plans(nopp, ndeal):
                    got = P.positions(n_plan, rule, d, paired=True)
                    bad = np.flatnonzero((got != want).any(1))
                    assert len(bad) == 0, ((nopp, ndeal), rule, n_plan, d[bad[0]], got[bad[0]], want[bad[0]])
                    assert np.array_equal(got, P.positions(n_plan, rule, d, paired=False)), ((nopp, ndeal), rule, n_plan)


# ---------------------------------------------------------------------------------------------------------- tallies
def form_rows(ci, uniform, ways, paired):
    nopp, ndeal = T.CELLS[ci]
    if nopp < 0:   # the general form does not deal by a plan: tests/hostsim_join names it
        return hostsim_join.rows(T.cell_queries(ci), T.SEED, T.FQ + ci * T.STATES, nopp, ndeal, uniform=uniform, ways=ways)
    return P.rows(T.cell_queries(ci), T.SEED, T.FQ + ci * T.STATES, nopp, ndeal, uniform=uniform, ways=ways, paired=paired)


@pytest.fixture(scope="module")
def want():
    """the oracle's rows of every cell's states, per law: computed once, read-only"""
    q = np.concatenate([np.ascontiguousarray(T.cell_queries(ci), np.uint8).reshape(-1, 16) for ci in range(len(T.CELLS))])
    out = {}
    for mode, _ in T.LAWS:
        w = O.run_batch(mode, q, T.SEED, first_qid=T.FQ, threads=8)
        w.setflags(write=False)
        out[mode] = w
    return out


@pytest.mark.parametrize("mode,uniform", T.LAWS, ids=["reference_law", "uniform_law"])
def test_plain_rows_equal_the_oracle_and_the_unpaired_text(want, mode, uniform):
    assert len(T.CELLS) == 31 and len(set(T.CELLS)) == 31
    for ci, (nopp, ndeal) in enumerate(T.CELLS):
        got = form_rows(ci, uniform, False, True)
        exp = want[mode][ci * T.STATES:(ci + 1) * T.STATES]
        assert int(got[:, 0].sum()) == T.STATES * T.RUNS
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, ((nopp, ndeal), bad[:4], got[bad[:2]], exp[bad[:2]])
        if nopp >= 1:
            assert np.array_equal(got, form_rows(ci, uniform, False, False)), (nopp, ndeal)


@pytest.mark.parametrize("mode,uniform", T.LAWS, ids=["reference_law", "uniform_law"])
def test_split_pot_rows_equal_the_oracle_and_the_unpaired_text(want, mode, uniform):
    """the thirteen plain words of a split-pot row are the oracle's; its tie_ways are those of the unpaired text, which
    tests/test_epoch_dealing_host.py holds against the dealing without plans"""
    for ci, (nopp, ndeal) in enumerate(T.CELLS):
        got = form_rows(ci, uniform, True, True)
        assert np.array_equal(got[:, :13], want[mode][ci * T.STATES:(ci + 1) * T.STATES]), (nopp, ndeal)
        assert np.array_equal(got[:, 13:].sum(1), got[:, 3]), (nopp, ndeal)
        if nopp >= 1:
            assert np.array_equal(got, form_rows(ci, uniform, True, False)), (nopp, ndeal)


def test_parity_forms_equal_the_mt_walk():
    """mcq_iterations_replay4: 1 to 5 opponents take straight forms that deal by the plan of five table cards (four and five
    opponents count a pair), six and more the general form"""
    rng = np.random.RandomState(2099)
    hole, board, npl = [], [], []
    for players in range(2, 9):
        for nb in (0, 3, 4, 5):
            for _ in range(3):
                deck = rng.permutation(52)
                hole.append(deck[:2])
                board.append(list(deck[2:2 + nb]) + [255] * (5 - nb))
                npl.append(players)
    for runs in (129, 1000):
        q = O.pack_queries(np.array(hole, np.uint8), np.array(board, np.uint8), np.array(npl), runs)
        exp = O.run_batch(O.MODE_MT, q, 5151, first_qid=T.FQ, threads=8)    # query i under the seed 5151 + FQ + i
        got = np.concatenate([P.replay_rows(q[i:i + 1], 5151 + T.FQ + i) for i in range(len(q))])
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, (runs, bad[:4], got[bad[:2]], exp[bad[:2]])


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- the primitive on every byte pair, plans of every rule on boundary rows with the switch on and off,
    iterations of a few forms, parity mode -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a
    program of its own."""
    lines = hostbuild.run_sanitized("hostsim_paired/hs_main.cpp", "-O0", tmp_path)
    assert lines[-1].startswith("ok:"), lines
