"""Test helper: the cases of the preflop hero-range exact enumeration (mcq_exact_batch_hero_range_preflop).

A case is tests/hero_range_cases.py's (hero range, opponent range, table cards, ghost cards) with an empty table; its
records(), allowed_hands() and hand_records() are used as they are.  The two decks: all 52 cards, and 50 cards with the two
highest (AH, AS) as ghost cards, so that D's top card is AD.
"""
import math

import numpy as np

from neuron_poker_amd import _lib
from tests import hero_range_cases as HC

GHOSTS = {52: None, 50: ["AH", "AS"]}
TOP10 = 0.10
NARROW_HERO = {"AA", "AKS"}                      # 10 hands of the full deck
HOST_HERO = {"AA", "AKS", "72O"}                 # 22 hands; AA and AKs hold D's highest card
OPP_3CLS = {"KK", "QQ", "AKO"}
SLICE = 3000


def case(hero, opp, n_deck=52):
    return (hero, opp, [], GHOSTS[n_deck])


def n_boards(n_deck):
    return math.comb(n_deck, 5)


def slices(n_deck):
    """[lo, hi) of the three completion slices: the first 3000, 3000 from the middle, the last 3000."""
    n = n_boards(n_deck)
    return [(0, SLICE), (n // 2 - SLICE // 2, n // 2 - SLICE // 2 + SLICE), (n - SLICE, n)]


def unrank(idx, n, k):
    """Index -> k ascending positions below n in the combinatorial number system: idx = sum C(pos[i], i + 1)."""
    pos = [0] * k
    c = n
    for i in range(k, 0, -1):
        c -= 1
        while math.comb(c, i) > idx:
            c -= 1
        pos[i - 1] = c
        idx -= math.comb(c, i)
    assert idx == 0
    return pos


def rank(pos):
    return sum(math.comb(p, i + 1) for i, p in enumerate(pos))


def opp_bits(c):
    b = HC.parts(c)[1]
    return np.asarray(_lib.ALL_CLASSES if b is None else b, np.uint32)


def boundary_hands(n_deck=52):
    """Eight hero hands of the unrestricted range, as rows: the first and the last row, the hands at positions 1023 and
    1024 of the `allowed` list (the last thread of the first group of blocks and the first of the second) and four in
    between.  With every class allowed and D = the lowest n_deck cards, list position = D-pair index = row."""
    last = n_deck * (n_deck - 1) // 2 - 1
    return [0, 1, 511, 1023, 1024, 1025, last - 1, last]


ROW_HANDS = [(a, b) for b in range(52) for a in range(b)]   # row -> (a, b)
