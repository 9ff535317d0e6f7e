"""(hero, table) situations in which rare hand shapes are COMMON -- shared by the hot-board tests of every Monte-Carlo
kernel.  Random heroes and tables meet a straight flush against a higher flush of the same suit, quads on the table or
a wheel a few times in thousands of iterations; here every iteration of a situation is about that shape.  Each
situation runs at 2, 6 and 10 players.  tests/test_hot_boards_host.py proves from the oracle alone that the list does
what it claims (every by_type column used, the three rarest types and ties frequent)."""
import numpy as np

from oracle import oracle as O

SITUATIONS = [
    # four to a straight flush on the turn
    (["AH", "AD"], ["6S", "7S", "8S", "9S"]),            # open-ended
    (["KH", "KD"], ["5H", "6H", "8H", "9H"]),            # gut-shot
    (["KC", "QD"], ["AS", "2S", "3S", "4S"]),            # the wheel
    (["2C", "2D"], ["TS", "JS", "QS", "KS"]),            # broadway
    # a royal / straight flush on the river table
    (["AC", "AD"], ["TS", "JS", "QS", "KS", "AS"]),
    (["TD", "2C"], ["5D", "6D", "7D", "8D", "9D"]),      # hero holds the card above it
    (["4D", "KC"], ["5D", "6D", "7D", "8D", "9D"]),      # ... the card below it
    # a five-flush table, hero holding a higher and a lower card of the suit
    (["AC", "3C"], ["2C", "7C", "9C", "JC", "KC"]),
    # quads on the table: the reference scores them by the two highest distinct ranks of all seven cards
    (["AH", "2D"], ["9C", "9D", "9H", "9S"]),            # hero above the quads
    (["3H", "2D"], ["9C", "9D", "9H", "9S"]),            # hero below
    (["KH", "2D"], ["9C", "9D", "9H", "9S", "5C"]),
    # trips + pair and two pairs on the table
    (["AH", "KD"], ["7C", "7D", "7H", "4S", "4C"]),
    (["AH", "QD"], ["8C", "8D", "5H", "5S"]),
    # a monotone and a paired flop
    (["AH", "KH"], ["2H", "7H", "9H"]),
    (["9H", "4D"], ["9C", "9D", "4S"]),
    # three pairs in seven cards
    (["5C", "5D"], ["8C", "8D", "JH", "JS"]),
    # a wheel on the table, hero holding a six
    (["6C", "KD"], ["AD", "2C", "3H", "4S", "5D"]),
    # and the headline instance's street: before the flop
    (["AS", "KS"], []),
]
PLAYERS = (2, 6, 10)
RUNS = 3000          # three tasks, the last one partly filled; not a multiple of 16
SEED, MT_SEED, QID = (1 << 41) | 0x51ED270B, 0x2545F491, 77
# one ranged opponent: pairs, suited broadway, the big off-suit aces
RANGE = [r + r for r in "23456789TJQKA"] + [a + b + "S" for i, a in enumerate("TJQKA") for b in "TJQKA"[:i]] + ["AKO", "AQO", "KQO"]


def cases():
    return [(h, t, n) for h, t in SITUATIONS for n in PLAYERS]


def queries(runs=RUNS):
    """the list as 16-byte query records (numpy uint8 [n, 16])"""
    cs = cases()
    hole = [[O.card_id(c) for c in h] for h, _, _ in cs]
    board = [[O.card_id(c) for c in t] + [255] * (5 - len(t)) for _, t, _ in cs]
    return O.pack_queries(hole, board, [n for _, _, n in cs], runs)


def expected(mode, runs=RUNS, threads=8):
    """oracle rows [n, 13]; query i runs under id QID + i (MODE_MT: under the seed MT_SEED + QID + i)"""
    return O.run_batch(mode, queries(runs), MT_SEED if mode == O.MODE_MT else SEED, first_qid=QID, threads=threads)


def grid_queries(rng, runs=1025):
    """one random query in each of the 40 (players 1..10) x (preflop, flop, turn, river) cells = kernel instances"""
    hole, board, npl = [], [], []
    for p in range(1, 11):
        for nb in (0, 3, 4, 5):
            c = rng.permutation(52)[:2 + nb]
            hole.append(c[:2])
            board.append(list(c[2:]) + [255] * (5 - nb))
            npl.append(p)
    return O.pack_queries(hole, board, npl, runs)
