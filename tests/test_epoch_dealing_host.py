"""Dealing in epochs (mcq_deal_plan, mcq_draw_epoch; the straight forms of mcq_iteration_sum deal by it), without a GPU.

tests/hostsim_epochs builds the lane code for the host with the instantiation named by the caller.

* Positions against list.pop.  Explicit draws, as parity mode's draw policy hands them over, through the dealing of every
  plan built (at most one, two, three checkpoints; a checkpoint at every full register), for 1 to 9 opponents x 0 to 5 table
  cards to come -- by the plan of exactly those draws and, as the forms that count the table cards at run time deal, by
  the plan of five table cards stopped early.  Expected: Python's list.pop on the ordered deck of 45 + n_deal cards.
  The rows: all zeros; every draw the last index of its list; strictly rising; strictly falling; every draw equal to, one
  below or one above the one before it (a hole's t == r and t == r + 1 on both sides of every checkpoint); 100 000 random
  rows per shape (expected rows from list.pop written with numpy, itself checked against list.pop on the first rows).
* Tallies against the oracle.  Every straight instantiation (1 to 7 opponents x 5, 2, 1 cards to come or a run-time count, 8
  and 9 opponents with a run-time count) under the rule the product ships, and the general form, which deals as before
  -- 31 forms, both accumulators, both laws, 64 random states each, against the oracle's CTR mode; the straight forms also
  against the same text dealing without plans (rule 0).  Parity mode's straight forms (1 to 5 opponents) against the
  oracle's MT19937 mode.
* The same lane code in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hostbuild
from tests import hostsim_epochs as E
from tests import hostsim_join

SHAPES = [(nopp, ndeal) for nopp in range(1, 10) for ndeal in range(0, 6)]
N_RANDOM = 100000


def list_pop_rows(draws, deck_len):
    """list.pop itself, row by row"""
    out = np.zeros_like(draws)
    for i, row in enumerate(draws):
        deck = list(range(deck_len))
        for j, r in enumerate(row):
            out[i, j] = deck.pop(int(r))
    return out


def list_pop_numpy(draws, deck_len):
    """the same for many rows: the deck of every row as an array, the popped entry closed up"""
    rows, n = draws.shape
    deck = np.broadcast_to(np.arange(deck_len, dtype=np.uint8), (rows, deck_len)).copy()
    out = np.zeros_like(draws)
    ar = np.arange(rows)
    for j in range(n):
        r = draws[:, j].astype(np.intp)
        out[:, j] = deck[ar, r]
        deck = np.where(np.arange(deck.shape[1] - 1)[None, :] < r[:, None], deck[:, :-1], deck[:, 1:])
    return out


def pattern_rows(n, deck_len):
    """the rows that can break an epoch boundary; every entry j is a valid index of a list of deck_len - j cards"""
    top = deck_len - 1 - np.arange(n)                     # the last index of every list
    j = np.arange(n)
    rows = [np.zeros(n, int), top.copy()]
    rows += [j + c for c in (0, 1, 5) if (j + c <= top).all()]                    # strictly rising
    rows += [(n - 1 - j) * s + c for s in (1, 2) for c in (0, 3) if ((n - 1 - j) * s + c <= top).all()]   # strictly falling
    for base in (0, 1, 7, int(top.min()) - 1):
        for j0 in range(1, n):
            for d in (-1, 0, 1):                           # all equal, and draw j0 one below / equal / one above
                row = np.full(n, base)
                row[j0:] += d
                for d2 in (-1, 1):                         # ... and the draw behind it moving once more
                    row2 = row.copy()
                    row2[j0 + 1:] += d2
                    rows += [row, row2]
    rng = np.random.RandomState(n * 64 + deck_len)         # random walks of steps -1, 0, +1
    walk = np.cumsum(rng.randint(-1, 2, size=(400, n)), axis=1) + rng.randint(0, 20, size=(400, 1))
    rows += list(walk)
    rows = np.array([r for r in rows if (r >= 0).all() and (r <= top).all()])
    return np.unique(rows, axis=0).astype(np.uint8)


def shape_plans(nopp, ndeal):
    """(draws of the plan) a form of this shape may deal by: its own count, and the count with five table cards"""
    return sorted({2 * nopp + ndeal, 2 * nopp + 5})


def test_plans_are_valid_and_cost_what_the_model_says():
    for n in range(2, 24):
        for rule in E.RULES:
            p = E.plan(n, rule)
            assert p["valid"] and p["reg0"][-1] <= 6, (n, rule, p)
            cps = [0] + p["checkpoints"] + [n]
            assert all(a < b for a, b in zip(cps, cps[1:])), (n, rule, p)
            if rule != E.FULLREG:
                assert len(p["checkpoints"]) <= rule
                if rule > 1:
                    assert p["cost"] <= E.plan(n, rule - 1)["cost"]
            else:
                assert p["checkpoints"] == list(range(4, n, 4))
    six_max = {1: ([8], 148), 2: ([8, 12], 145), 3: ([8, 12, 13], 143), E.FULLREG: ([4, 8, 12], 146)}
    for rule, (cps, cost) in six_max.items():
        p = E.plan(15, rule)
        assert (p["checkpoints"], p["cost"]) == (cps, cost), (rule, p)
    assert E.plan(23, 3)["cost"] == 308 and E.plan(12, 3)["cost"] == 98 and E.plan(11, 3)["cost"] == 82
    assert E.shipped_rule() in E.RULES


@pytest.mark.parametrize("rule", E.RULES)
def test_pattern_rows_equal_list_pop(rule):
    for nopp, ndeal in SHAPES:
        n, deck_len = 2 * nopp + ndeal, 45 + ndeal
        d = pattern_rows(n, deck_len)
        assert len(d) >= 50 and (d == 0).all(1).any() and (d == deck_len - 1 - np.arange(n)).all(1).any()
        want = list_pop_rows(d, deck_len)
        for n_plan in shape_plans(nopp, ndeal):
            got = E.positions(n_plan, rule, d)
            bad = np.flatnonzero((got != want).any(1))
            assert len(bad) == 0, ((nopp, ndeal), n_plan, d[bad[0]], got[bad[0]], want[bad[0]])


def test_random_rows_equal_list_pop():
    """100 000 random rows per shape: a row of the ten-player shape, cut behind 2 * n_opp + n_deal draws, is a random row
    of the shape with fewer opponents (draw j is uniform on the deck_len - j cards left, whoever takes the card), so the
    expected positions are worked out once per number of table cards"""
    rng = np.random.RandomState(20817)
    for ndeal in range(0, 6):
        deck_len, n_max = 45 + ndeal, 18 + ndeal
        d_all = (rng.randint(0, 1 << 30, size=(N_RANDOM, n_max)) % (deck_len - np.arange(n_max))).astype(np.uint8)
        want_all = list_pop_numpy(d_all, deck_len)
        assert np.array_equal(want_all[:300], list_pop_rows(d_all[:300], deck_len))
        for nopp in range(1, 10):
            n = 2 * nopp + ndeal
            d, want = np.ascontiguousarray(d_all[:, :n]), want_all[:, :n]
            for rule in E.RULES:
                for n_plan in shape_plans(nopp, ndeal):
                    got = E.positions(n_plan, rule, d)
                    bad = np.flatnonzero((got != want).any(1))
                    assert len(bad) == 0, ((nopp, ndeal), rule, n_plan, d[bad[0]], got[bad[0]], want[bad[0]])


def test_a_plan_refuses_more_draws_than_it_has():
    with pytest.raises(ValueError):
        E.positions(7, 2, np.zeros((1, 8), np.uint8))
    with pytest.raises(ValueError):
        E.positions(24, 2, np.zeros((1, 8), np.uint8))
    with pytest.raises(ValueError):
        E.positions(15, 5, np.zeros((1, 8), np.uint8))


# ---------------------------------------------------------------------------------------------------------- tallies
SEED, FQ = (1 << 45) | 0xE70C5, 23
STATES, RUNS = 64, 256
CELLS = [(n, d) for n in range(1, 8) for d in (5, 2, 1, -1)] + [(8, -1), (9, -1), (-1, -1)]
BOARDS = (5, 4, 3, 0)   # table cards of a state where the cards to come are counted at run time
LAWS = [(O.MODE_CTR, False), (O.MODE_CTR_UNIFORM, True)]


def cell_queries(ci):
    nopp, ndeal = CELLS[ci]
    rng = np.random.RandomState(7000 + ci)
    hole, board, npl = [], [], []
    for i in range(STATES):
        deck = rng.permutation(52)
        nb = 5 - ndeal if ndeal >= 0 else BOARDS[i % 4]
        hole.append(deck[:2])
        board.append(list(deck[2:2 + nb]) + [255] * (5 - nb))
        npl.append(nopp + 1 if nopp >= 0 else 1 + (i // 4) % 10)   # the general form: hero alone up to ten players
    return O.pack_queries(np.array(hole, np.uint8), np.array(board, np.uint8), np.array(npl), RUNS)


def form_rows(ci, uniform, ways, planned=True):
    nopp, ndeal = CELLS[ci]
    if nopp < 0:   # the general form deals as before: tests/hostsim_join names it
        return hostsim_join.rows(cell_queries(ci), SEED, FQ + ci * STATES, nopp, ndeal, uniform=uniform, ways=ways)
    return E.rows(cell_queries(ci), SEED, FQ + ci * STATES, nopp, ndeal, uniform=uniform, ways=ways, planned=planned)


@pytest.fixture(scope="module")
def want():
    """the oracle's rows of every cell's states, per law: computed once, read-only"""
    q = np.concatenate([np.ascontiguousarray(cell_queries(ci), np.uint8).reshape(-1, 16) for ci in range(len(CELLS))])
    out = {}
    for mode, _ in LAWS:
        w = O.run_batch(mode, q, SEED, first_qid=FQ, threads=8)
        w.setflags(write=False)
        out[mode] = w
    return out


@pytest.mark.parametrize("mode,uniform", LAWS, ids=["reference_law", "uniform_law"])
def test_plain_rows_equal_the_oracle(want, mode, uniform):
    assert len(CELLS) == 31 and len(set(CELLS)) == 31
    for ci, (nopp, ndeal) in enumerate(CELLS):
        got = form_rows(ci, uniform, False)
        exp = want[mode][ci * STATES:(ci + 1) * STATES]
        assert int(got[:, 0].sum()) == STATES * RUNS
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, ((nopp, ndeal), bad[:4], got[bad[:2]], exp[bad[:2]])


@pytest.mark.parametrize("mode,uniform", LAWS, ids=["reference_law", "uniform_law"])
def test_split_pot_rows_equal_the_oracle_and_the_dealing_without_plans(want, mode, uniform):
    """the thirteen plain words of a split-pot row are the oracle's; its tie_ways are those of the same text dealing without
    plans, which tests/test_late_join_host.py holds against a recount of the oracle's trace"""
    seen = np.zeros(9, np.uint64)
    for ci, (nopp, ndeal) in enumerate(CELLS):
        got = form_rows(ci, uniform, True)
        assert np.array_equal(got[:, :13], want[mode][ci * STATES:(ci + 1) * STATES]), (nopp, ndeal)
        assert np.array_equal(got[:, 13:].sum(1), got[:, 3]), (nopp, ndeal)
        if nopp >= 1:
            assert np.array_equal(got, form_rows(ci, uniform, True, planned=False)), (nopp, ndeal)
            assert np.array_equal(got, hostsim_join.rows(cell_queries(ci), SEED, FQ + ci * STATES, nopp, ndeal,
                                                         uniform=uniform, ways=True)), (nopp, ndeal)
        seen += got[:, 13:].sum(0)
    assert int((seen != 0).sum()) >= 3, seen   # pots shared two, three and more ways occur


def test_parity_forms_equal_the_mt_walk():
    """mcq_iterations_replay4: 1 to 5 opponents take straight forms that deal by the plan of five table cards, six and more
    the general form"""
    rng = np.random.RandomState(99)
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
        exp = O.run_batch(O.MODE_MT, q, 4242, first_qid=FQ, threads=8)    # query i under the seed 4242 + FQ + i
        got = np.concatenate([E.replay_rows(q[i:i + 1], 4242 + FQ + i) for i in range(len(q))])
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, (runs, bad[:4], got[bad[:2]], exp[bad[:2]])


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp -- plans of every rule on boundary rows, iterations of a few forms, parity mode -- built with
    AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
    lines = hostbuild.run_sanitized("hostsim_epochs/hs_main.cpp", "-O0", tmp_path)
    assert lines[-1].startswith("ok:"), lines
