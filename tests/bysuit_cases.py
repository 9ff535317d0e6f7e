"""The states of tests/test_hole_by_suit_host.py and tests/test_hole_by_suit_gpu.py: one query per cell of 2 to 10 players x
0, 3, 4, 5 known table cards, chosen for what the flush suit of the table can be when the opponents' cards are read by it.

A card is 4 * rank + suit, suits 0..3 = clubs, diamonds, hearts, spades.  The known table cards, by the suits they hold:
  flop   three clubs, three diamonds, three hearts, three spades (the suit is decided before anything is dealt), a rainbow
         flop (no suit yet: turn and river can still make one), then the four one-suit flops again with other heroes;
  turn   2 + 2 clubs and diamonds (the suit is decided only on the river), a four-flush of every suit, 2 + 2 hearts and
         spades, three hearts and a club, three spades and a diamond, 2 + 1 + 1;
  river  three of every suit with two others, four clubs, four spades, five hearts, 2 + 2 + 1 (no flush: suit 0 is read).
Hero holds zero, one and two cards of the table's most frequent suit in turn; before the flop hero is suited and off suit
in turn.
"""
import numpy as np

RANKS = [7, 8, 0, 11, 3]                     # 9 T 2 K 5: the table's ranks, in order
HERO_RANKS = [12, 10]                        # A Q: never on the table
FLOPS = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [0, 1, 2], [0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]]
TURNS = [[0, 1, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [2, 3, 3, 2], [2, 2, 0, 2], [3, 1, 3, 3], [0, 1, 2, 0]]
RIVERS = [[0, 0, 1, 0, 2], [1, 3, 1, 1, 0], [2, 2, 2, 0, 1], [3, 0, 3, 1, 3], [0, 0, 0, 1, 0], [3, 3, 2, 3, 3], [2, 2, 2, 2, 2],
          [0, 1, 0, 1, 2], [3, 2, 3, 2, 1]]
SUITS = {0: [[]] * 9, 3: FLOPS, 4: TURNS, 5: RIVERS}


def cells():
    """[(hole, board, players, table's suit or None, hero's cards of it)] in the order players 2..10 x table cards 0, 3, 4, 5"""
    out = []
    for p in range(2, 11):
        for nb in (0, 3, 4, 5):
            suits = SUITS[nb][p - 2]
            board = [4 * RANKS[i] + s for i, s in enumerate(suits)]
            if nb == 0:
                t, k = None, None
                hole = [4 * HERO_RANKS[0] + p % 4, 4 * HERO_RANKS[1] + (p % 4 if p % 2 else (p + 1) % 4)]
            else:
                t = max(range(4), key=lambda s: (suits.count(s), -s))
                k = (p + nb) % 3
                other = (t + 1) % 4
                hole = [4 * HERO_RANKS[i] + (t if i < k else other) for i in range(2)]
            assert len(set(hole + board)) == 2 + nb
            out.append((hole, board, p, t, k))
    return out


def pack(cell_list, runs, pack_queries):
    hole = np.array([c[0] for c in cell_list], np.uint8)
    board = np.array([list(c[1]) + [255] * (5 - len(c[1])) for c in cell_list], np.uint8)
    return pack_queries(hole, board, np.array([c[2] for c in cell_list]), runs)


def check_coverage(cell_list):
    """what the cases claim, asserted: called by both test files"""
    assert len(cell_list) == 36 and len({(c[2], len(c[1])) for c in cell_list}) == 36
    suit_of = lambda c: [x % 4 for x in c[1]]
    flops = [suit_of(c) for c in cell_list if len(c[1]) == 3]
    for s in range(4):
        assert [s, s, s] in flops                                               # three of every suit in turn
    assert any(len(set(f)) == 3 for f in flops)                                 # a rainbow flop
    turns = [sorted(suit_of(c)) for c in cell_list if len(c[1]) == 4]
    assert [0, 0, 1, 1] in turns and [2, 2, 3, 3] in turns                      # 2 + 2: decided on the river
    for s in range(4):
        assert [s] * 4 in turns                                                 # a four-flush turn
    rivers = [suit_of(c) for c in cell_list if len(c[1]) == 5]
    assert {max(r.count(s) for s in range(4)) for r in rivers} == {2, 3, 4, 5}
    assert {s for r in rivers for s in range(4) if r.count(s) >= 3} == {0, 1, 2, 3}
    held = {(len(c[1]), c[4]) for c in cell_list if c[3] is not None}
    assert held == {(nb, k) for nb in (3, 4, 5) for k in (0, 1, 2)}             # hero: zero, one, two cards of the suit
    for c in cell_list:
        if c[3] is not None:
            assert sum(1 for x in c[0] if x % 4 == c[3]) == c[4]
    pre = [c[0] for c in cell_list if not c[1]]
    assert any(a % 4 == b % 4 for a, b in pre) and any(a % 4 != b % 4 for a, b in pre)
