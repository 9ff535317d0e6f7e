"""The production dealing law (MCQ_MODE_PHILOX, the MCQ-CTR streams) IS the reference's law at 4-10 players, on the GPU.

The kernels equal the oracle's CTR mode bit for bit elsewhere; these tests pin that specification to the reference's
law as a law, where the headline workload lives (six players), with tests/lawstats.py: win, tie and the nine winning
hand types, one bound of 5.5 sigma, fixed seeds.
(a) plain queries, players 4, 5, 6, 8, 10 x every street x three hero hands (two of them hold the deck's highest card
    ids, where the index bias acts): production against replay mode (the reference's MT19937 stream, bit-exact to it),
    1e9 iterations per side and cell (1000 queries x 1e6);
(b) in the same cells, production under the uniform law: in every cell chosen for it (all but the river cells of AsKs,
    where the two laws lie closest: 12 sigma apart at 10 players) |reference - uniform| must exceed 4 x the bound
    (measured: 128-4700 sigma), so a law error of the index bias's size cannot pass (a);
(c) extended queries of 4-10 seats (2-7 known hands, 0-2 random opponents, unrestricted / top-25 % / a small set
    range, with and without ghost cards) against exact enumeration (Engine.exact_ext): 4e8 iterations through the
    general path and 1.05e8 through the one-launch path (mcq_eval_ext_small_kernel, 8 queries of 8192 per call).
    The uniform law is enumerated exactly but the extended kernels deal the reference's law only, so production
    refuses extended queries under it (ValueError) instead of dealing the wrong law under its name;
(d) extended queries that exact enumeration refuses (3-5 ranged random opponents, a hero range, a ranged known hand)
    at 4-8 players: production against replay mode, 1e8 iterations per side.
Measured on one MI355X: 43 s for the file.  (a) + (b) 2.2 s at 4 players to 18.6 s at 10, nearly all of it the replay
side; (c) and (d) at most 0.2 s per case.  Largest |z| of a law comparison: 3.2 (of 65 in (a), 20 in (c), 5 in (d)).
"""
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from neuron_poker_amd.cards import card_id
from tests import lawstats as L

pytestmark = pytest.mark.gpu

TOP25 = mh._opponent_range_bits(0.25)
TOP50 = mh._opponent_range_bits(0.5)
PAIRS_AK = _lib.range_bits({"AA", "KK", "AKS", "AKO", "QQ"})   # a small set range with neighbour pairs (AcAd, ...)


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def _ids(cards):
    return [card_id(c) for c in cards]


# ------------------------------------------------------------------------------ (a) + (b): plain queries, 4-10 players
BOARD = ["2C", "7D", "9S", "JH", "QC"]
HEROES = [["AS", "AH"], ["AS", "KS"], ["7C", "2D"]]
QUERIES, RUNS = 1000, 1_000_000                                   # per cell and side: 1e9 iterations


def _sensitive(nb, hero):
    return not (nb == 5 and hero == ["AS", "KS"])


@pytest.mark.parametrize("n_players", [4, 5, 6, 8, 10])
def test_plain_production_law_is_the_reference_law(eng, n_players):
    cells = [(nb, hero) for nb in (0, 3, 4, 5) for hero in HEROES]
    q = np.concatenate([np.repeat(_lib.pack_query_one(_ids(hero), _ids(BOARD[:nb]), n_players, RUNS), QUERIES)
                        for nb, hero in cells])
    t0 = time.time()
    rep = eng.eval_batch(q, seed=10_000_000 * n_players, mode=npa.MODE_REPLAY_MT19937)   # seeds 1e7 n + query index
    t1 = time.time()
    ctr = eng.eval_batch(q, seed=20261016 + n_players)
    t2 = time.time()
    eng.set_dealing_law("uniform")
    try:
        uni = eng.eval_batch(q, seed=20261116 + n_players)
    finally:
        eng.set_dealing_law("reference")
    print("%d players, %d cells x %.0e iterations: replay %.1f s, production %.1f s, uniform %.1f s"
          % (n_players, len(cells), QUERIES * RUNS, t1 - t0, t2 - t1, time.time() - t2))
    for k, (nb, hero) in enumerate(cells):
        s = slice(k * QUERIES, (k + 1) * QUERIES)
        assert int(rep["runs"][s].sum()) == int(ctr["runs"][s].sum()) == int(uni["runs"][s].sum()) == QUERIES * RUNS
        label = "%dp %s %d board cards" % (n_players, "".join(hero), nb)
        L.check(label + ", production vs replay", L.two_sample(ctr[s], rep[s]))
        d = L.two_sample(uni[s], rep[s])
        print(L.report(label + ", uniform vs replay", d))
        if _sensitive(nb, hero):
            assert L.max_z(d) > 4 * L.BOUND, (label, d)


# ------------------------------------------------------------------- (c): extended queries against exact enumeration
EXACT_CASES = [  # (id, hero, board, players, known hands, ghost, range): hero + known + random = players
    ("4s-known3-turn-0rand-ghost", ["AS", "KS"], BOARD[:4], 4, (["QH", "QD"], ["TC", "9C"], ["AH", "5D"]), ["2S", "3S"], None),
    ("8s-known7-preflop-0rand", ["AS", "AH"], [], 8,
     (["KS", "KH"], ["QC", "JC"], ["7D", "7H"], ["5S", "4S"], ["AD", "TH"], ["9D", "8D"], ["2H", "3H"]), None, None),
    ("4s-known2-flop-1rand-top25", ["AS", "KS"], BOARD[:3], 4, (["QH", "QD"], ["TC", "8C"]), None, TOP25),
    ("5s-known3-turn-1rand-set-ghost", ["KH", "KD"], BOARD[:4], 5, (["QS", "JS"], ["8C", "8D"], ["5H", "4H"]),
     ["AC", "3S"], PAIRS_AK),
    ("6s-known4-river-1rand-all", ["AS", "AH"], BOARD, 6, (["KS", "KH"], ["TD", "TS"], ["8H", "6H"], ["3C", "4C"]), None, None),
    ("6s-known4-preflop-1rand-top25-ghost", ["AS", "KS"], [], 6, (["QH", "QD"], ["7C", "2D"], ["JD", "TD"], ["5S", "5C"]),
     ["AD", "3H"], TOP25),
    ("7s-known4-flop-2rand-top25", ["AH", "KD"], BOARD[:3], 7, (["QH", "QD"], ["TC", "8C"], ["6S", "6H"], ["4D", "3D"]),
     None, TOP25),
    ("8s-known5-turn-2rand-set-ghost", ["7C", "2D"], BOARD[:4], 8,
     (["TH", "TS"], ["9C", "8C"], ["6S", "5S"], ["4H", "3H"], ["JD", "8D"]), ["2H", "3S"], PAIRS_AK),
    ("9s-known6-river-2rand-all-ghost", ["AS", "AH"], BOARD, 9,
     (["KS", "KH"], ["TD", "TS"], ["8H", "6H"], ["3C", "4C"], ["5D", "5S"], ["6C", "6D"]), ["KC", "KD"], None),
    ("10s-known7-flop-2rand-top25", ["AS", "KS"], BOARD[:3], 10,
     (["QH", "QD"], ["TC", "8C"], ["6S", "6H"], ["4D", "3D"], ["5S", "5C"], ["7H", "7S"], ["8H", "8S"]), None, TOP25),
]
GENERAL_QUERIES, GENERAL_RUNS = 100, 4_000_000                   # 4e8 iterations through mcq_eval_ext_kernel
SMALL_CALLS, SMALL_Q, SMALL_RUNS = 1600, 8, 8192                 # 1.05e8 through mcq_eval_ext_small_kernel


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_extended_production_law_is_the_exact_law(eng, case):
    name, hero, board, n, known, ghost, rng = case
    assert 4 <= n <= 10 and 2 <= len(known) <= 7 and 0 <= n - 1 - len(known) <= 2
    q = _lib.pack_query_one(_ids(hero), _ids(board), n, 1)
    e = _lib.pack_query_ext(1, ghost=_ids(ghost) if ghost else None, known=[_ids(h) for h in known], opp_range=rng)
    t0 = time.time()
    exact = {law: eng.exact_ext(q, e, law)[0][0] for law in ("reference", "uniform")}
    t1 = time.time()
    qq = np.repeat(q, GENERAL_QUERIES)
    qq["runs"] = GENERAL_RUNS
    general = eng.eval_batch_ext(qq, np.repeat(e, GENERAL_QUERIES), seed=20261016)
    t2 = time.time()
    qs = np.repeat(q, SMALL_Q)
    qs["runs"] = SMALL_RUNS
    es = np.repeat(e, SMALL_Q)
    small = np.concatenate([eng.eval_batch_ext(qs, es, seed=20261017, first_query_id=SMALL_Q * k) for k in range(SMALL_CALLS)])
    t3 = time.time()
    print("%s: exact (both laws) %.2f s, general path %.2f s, one-launch path %.2f s" % (name, t1 - t0, t2 - t1, t3 - t2))
    assert int(general["runs"].sum()) == GENERAL_QUERIES * GENERAL_RUNS
    assert int(small["runs"].sum()) == SMALL_CALLS * SMALL_Q * SMALL_RUNS
    L.check(name + ", general path vs exact", L.one_sample(general, exact["reference"]))
    L.check(name + ", one-launch path vs exact", L.one_sample(small, exact["reference"]))
    # the extended kernels deal the reference's law only: under the uniform law both paths refuse
    assert abs(sum(L.exact_vector(exact["uniform"])[2:]) - sum(L.exact_vector(exact["uniform"])[:2])) < 1e-12
    eng.set_dealing_law("uniform")
    try:
        with pytest.raises(ValueError, match="uniform dealing law"):
            eng.eval_batch_ext(qq[:1], e, seed=1)
        with pytest.raises(ValueError, match="uniform dealing law"):
            eng.eval_batch_ext(qs, es, seed=1)
    finally:
        eng.set_dealing_law("reference")
    r = eng.eval_batch_ext(qs[:1], es[:1], seed=1)                 # the context deals again under the reference law
    assert int(r["runs"][0]) == SMALL_RUNS


# ----------------------------------------- (d): what exact enumeration refuses -- production against replay, 4-8 players
REPLAY_CASES = [  # (id, hero (cards or class bits), board, players, known hands (cards or class bits), ghost, range)
    ("4p-flop-3rand-top25", ["AS", "KS"], BOARD[:3], 4, (), None, TOP25),
    ("6p-turn-5rand-top50-ghost", ["AH", "AD"], BOARD[:4], 6, (), ["AC", "KC"], TOP50),
    ("5p-preflop-hero-range-4rand-top50", TOP25, [], 5, (), None, TOP50),
    ("8p-river-ranged-known-4rand-top25", ["7C", "2D"], BOARD, 8, (["KS", "KH"], TOP25, ["TD", "TS"]), None, TOP25),
    ("7p-flop-hero-range-ranged-known-3rand-set", PAIRS_AK, BOARD[:3], 7, (TOP50, ["8H", "8S"], ["6C", "5C"]), ["2H", "3H"],
     TOP25),
]
REPLAY_QUERIES, REPLAY_RUNS = 4000, 25_000                        # 1e8 iterations per side


def _is_range(h):
    return isinstance(h, np.ndarray) and h.size == 6


@pytest.mark.parametrize("case", REPLAY_CASES, ids=[c[0] for c in REPLAY_CASES])
def test_extended_production_law_is_the_replayed_law(eng, case):
    name, hero, board, n, known, ghost, rng = case
    assert 4 <= n <= 8 and n - 1 - len(known) >= 3
    q = _lib.pack_query_one([0, 1] if _is_range(hero) else _ids(hero), _ids(board), n, REPLAY_RUNS)
    if _is_range(hero):
        q["hole"] = 0
    e = _lib.pack_query_ext(1, ghost=_ids(ghost) if ghost else None, hero_range=hero if _is_range(hero) else None,
                            known=[h if _is_range(h) else _ids(h) for h in known], opp_range=rng)
    qq, ee = np.repeat(q, REPLAY_QUERIES), np.repeat(e, REPLAY_QUERIES)
    t0 = time.time()
    rep = eng.eval_batch_ext(qq, ee, seed=30_000_000 + 10_000 * n, mode=npa.MODE_REPLAY_MT19937)
    t1 = time.time()
    ctr = eng.eval_batch_ext(qq, ee, seed=20261018 + n)
    print("%s: replay %.2f s, production %.2f s" % (name, t1 - t0, time.time() - t1))
    assert int(rep["runs"].sum()) == int(ctr["runs"].sum()) == REPLAY_QUERIES * REPLAY_RUNS
    L.check(name + ", production vs replay", L.two_sample(ctr, rep))
