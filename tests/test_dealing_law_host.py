"""The production dealing law's SPECIFICATION against the reference's law at 4-10 players, without a GPU.

The oracle's CTR mode (oracle/mcq_oracle.c deal_iteration, mcqo_run_ex2 mode 1) is what the production kernels equal
bit for bit; its MT mode is the reference's own MT19937 walk, pinned to the reference by tests/golden.  Here the two are
compared as laws (tests/lawstats.py, 5.5 sigma on win, tie and the nine winning types):
* plain queries: players 4, 6 and 10, every street, 2e7 iterations per side and player count (5e6 per street); a law
  error that moves a share by about 1.8e-3 (5.5 sigma of the difference at a share of 0.5) fails.  The hero hands hold
  the deck's highest card ids, where the reference's index bias (the second index of a pair and every table index stop
  one short of the deck's end) acts;
* extended queries: three opponents drawn from the top quarter of the classes, and a hero range against five
  opponents, 4e6 iterations per side each (about 1.9e-3 at a share of 0.5).
Measured on an 8-core host: 34 s for the file (largest |z| 2.4).  Giving the CTR table draw the whole deck
(deal_iteration's n = d.n for the reference law) fails the preflop cells at |z| up to 300.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from neuron_poker_amd.montecarlo_hip import _class_order
from oracle import oracle as O
from tests import lawstats as L

THREADS = min(16, os.cpu_count() or 1)
BOARD = ["2C", "7D", "9S", "JH", "QC"]
HERO_BY_STREET = {0: ["AS", "AH"], 3: ["AS", "KS"], 4: ["AH", "AD"], 5: ["7C", "2D"]}
PLAIN_ITERS = 5_000_000          # per side and cell
PLAIN_QUERIES = 200              # queries per cell: work for every thread, distinct MT seeds / CTR query ids


@pytest.mark.parametrize("n_players", [4, 6, 10])
def test_ctr_law_equals_the_reference_walk(n_players):
    cells = []
    for nb, hero in HERO_BY_STREET.items():
        board = [O.card_id(c) for c in BOARD[:nb]] + [255] * (5 - nb)
        q = O.pack_queries(np.array([[O.card_id(c) for c in hero]] * PLAIN_QUERIES, np.uint8),
                           np.array([board] * PLAIN_QUERIES, np.uint8), n_players, PLAIN_ITERS // PLAIN_QUERIES)
        cells.append(("%dp %s %d board cards" % (n_players, "".join(hero), nb), q))
    q = np.concatenate([c[1] for c in cells])
    mt = O.run_batch(O.MODE_MT, q, 1000 * n_players, threads=THREADS)          # seeds 1000 n + query index
    ctr = O.run_batch(O.MODE_CTR, q, 20261016 + n_players, threads=THREADS)
    assert int(mt[:, 0].sum()) == int(ctr[:, 0].sum()) == 4 * PLAIN_ITERS
    for i, (label, _) in enumerate(cells):
        s = slice(i * PLAIN_QUERIES, (i + 1) * PLAIN_QUERIES)
        L.check(label, L.two_sample(ctr[s], mt[s]))


EXT_ITERS = 4_000_000
EXT_CALLS = 80


def _run_ex_split(mode, seed, **kw):
    """EXT_ITERS iterations of one extended query as EXT_CALLS calls (CTR: query ids 0.., MT: seeds seed + i)."""
    runs = EXT_ITERS // EXT_CALLS

    def one(i):
        if mode == O.MODE_MT:
            return O.run_ex(mode, runs=runs, seed=seed + i, **kw)["tallies"]
        return O.run_ex(mode, runs=runs, seed=seed, qid=i, **kw)["tallies"]

    with ThreadPoolExecutor(THREADS) as pool:          # ctypes releases the GIL for the call
        return np.stack(list(pool.map(one, range(EXT_CALLS))))


TOP25 = set(_class_order()[-42:])
EXT_CASES = [
    ("4p flop, three opponents top-25 %", dict(hero=["AS", "KS"], board=BOARD[:3], n_players=4, opp_range=TOP25)),
    ("6p turn, hero range top-25 %", dict(hero=TOP25, board=BOARD[:4], n_players=6)),
]


@pytest.mark.parametrize("label,kw", EXT_CASES, ids=[c[0] for c in EXT_CASES])
def test_ctr_law_of_extended_queries_equals_the_reference_walk(label, kw):
    mt = _run_ex_split(O.MODE_MT, 7000, **kw)
    ctr = _run_ex_split(O.MODE_CTR, 20261016, **kw)
    assert int(mt[:, 0].sum()) == int(ctr[:, 0].sum()) == EXT_ITERS
    L.check(label, L.two_sample(ctr, mt))
