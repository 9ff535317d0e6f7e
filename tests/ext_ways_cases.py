"""Cases and expectations shared by the extended split-pot tests (host and GPU).

The oracle has no per-iteration trace for extended queries, so the expected 22-word rows come from four independent
checks together: (1) words 0..12 are the oracle's tallies (oracle.run_ex); (2) the nine further words are RECOUNTED here
from the hands the host build of the lane code dealt, with the oracle's own comparison (oracle.compare), as
tests/ways_expect.py does from the oracle's trace for plain queries; (3) the fast form equals the general form and an
extension record that restricts nothing equals the plain split-pot row; (4) the exact enumeration's weights equal a
literal walk in fractions (tests/exact_ways_literal.py) and the Monte-Carlo rows converge to them."""
import json
import os

import numpy as np

import neuron_poker_amd as npa
from oracle import oracle as O

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def top_classes(frac):
    with open(os.path.join(_ROOT, "neuron_poker_amd", "preflop_classes.json")) as f:
        order = json.load(f)
    return order[-int(169 * frac):]


# hero / known entries: two cards, or a set of class strings (a range); opp: class strings or None (every class)
CASES = [
    dict(name="royal_board_top50", hero=["2C", "3D"], board=["TS", "JS", "QS", "KS", "AS"], n=6, opp=top_classes(0.5)),
    dict(name="quads_board_known", hero=["2C", "3D"], board=["KC", "KD", "KH", "KS"], n=6, known=[["4H", "5D"]]),
    dict(name="three_ak_preflop", hero=["AH", "KD"], board=[], n=4, known=[["AS", "KC"], ["AD", "KH"]]),
    # (the case as first written down had 4 players; it cannot be dealt -- see UNDEALABLE -- and runs heads-up here)
    dict(name="aq_vs_aq_ak", hero=["AC", "QD"], board=["AD", "AH", "KS"], n=2, opp=["AQO", "AQS", "AKO"]),
    dict(name="hero_range", hero={"AKS", "AKO", "QQ"}, board=[], n=3),
    dict(name="ranged_known_robs", hero=["2C", "2D"], board=[], n=4, known=[{"AKS", "AKO"}, ["AS", "KS"]]),
    dict(name="ghost", hero=["AH", "KH"], board=["QH", "JH", "2C"], n=3, ghost=["AS", "AD"]),
]
# Hero AC QD on AD AH KS leaves ONE ace in the deck and every allowed class needs one: a second ranged opponent cannot be
# dealt.  With 4 players this query is the tests' undealable range (every path must raise, not hang).
UNDEALABLE = dict(name="aq_vs_aq_ak_4", hero=["AC", "QD"], board=["AD", "AH", "KS"], n=4, opp=["AQO", "AQS", "AKO"])
# cases with at most one random opponent and nothing the exact enumeration refuses (no hero range, no ranged known hand)
EXACT_CASES = [2, 3]
SEED, QID = 11, 5


def _is_range(h):
    return isinstance(h, (set, frozenset))


def records(case, runs):
    """-> (mcq_query record [1], mcq_query_ext record [1]) of a case."""
    hero = case["hero"]
    hole = [0, 1] if _is_range(hero) else [npa.card_id(c) for c in hero]
    b = [npa.card_id(c) for c in case["board"]]
    q = npa.pack_queries([hole], [b + [255] * (5 - len(b))], case["n"], runs)
    known = [npa.range_bits(h) if _is_range(h) else [npa.card_id(c) for c in h] for h in case.get("known", [])]
    ext = npa.pack_query_ext(1, ghost=[npa.card_id(c) for c in case["ghost"]] if case.get("ghost") else None, known=known,
                             hero_range=npa.range_bits(hero) if _is_range(hero) else None,
                             opp_range=npa.range_bits(case["opp"]) if case.get("opp") is not None else None)
    return q, ext


def oracle_tallies(mode, case, runs, seed=SEED, qid=QID):
    """Words 0..12 from the oracle.  mode: O.MODE_MT (the library seeds query qid with (seed + qid) mod 2^32) / O.MODE_CTR."""
    if mode == O.MODE_MT:
        seed, qid = (seed + qid) & 0xFFFFFFFF, 0
    hero = case["hero"]
    r = O.run_ex(mode, sorted(hero) if _is_range(hero) else hero, case["board"], case["n"], runs, seed, qid,
                 ghost=case.get("ghost"), opp_range=case.get("opp"),
                 known=[sorted(h) if _is_range(h) else h for h in case.get("known", [])])
    return r["tallies"].astype(np.uint64)


def recount(hands, n_players):
    """ways[k - 2], k = 2..10, and (win, tie) recounted from the dealt hands [runs, 2 n + 5] with oracle.compare."""
    ways = np.zeros(11, np.uint64)
    for row in hands:
        table = [int(c) for c in row[2 * n_players:]]
        seven = [[int(row[2 * p]), int(row[2 * p + 1])] + table for p in range(n_players)]
        cmp = [O.compare(seven[p], seven[0]) for p in range(1, n_players)]   # > 0: the other hand is greater
        if not any(c > 0 for c in cmp):
            ways[1 + sum(1 for c in cmp if c == 0)] += 1
    assert not ways[n_players + 1:].any()
    return ways[2:].copy(), int(ways[1]), int(ways[2:].sum())


_rows = {}


def hostsim_row(i, runs, replay, general=False, seed=SEED, qid=QID):
    """The host lane build's 22-word row of case i (cached: computed once, shared by the tests)."""
    from tests import hostsim_ext_ways as H
    key = (i, runs, replay, general, seed, qid)
    if key not in _rows:
        q, ext = records(CASES[i], runs)
        s = (seed + qid) & 0xFFFFFFFF if replay else seed
        _rows[key] = H.run(replay, q, ext, s, 0 if replay else qid, general=general)
    return _rows[key]


def assert_cases_vary(rows):
    """The cases must exercise what they claim: at least three distinct k >= 3 occur among them."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 22)
    assert int((rows[:, 14:22].sum(0) != 0).sum()) >= 3, rows[:, 13:22]
