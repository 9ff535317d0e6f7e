"""Cases shared by the exact per-seat tests with one random opponent (host and GPU): (hands, board, ghost, opp) -- hands[0]
is the hero, the rest the known hands, then ONE random opponent drawn from the classes `opp` (None: every class)."""
import numpy as np

import neuron_poker_amd as npa
from tests import ext_ways_cases as XC
from tests.seats_expect import ids

TOP25 = XC.top_classes(0.25)

HU_RIVER = ([["AH", "KD"]], ["2C", "7D", "9H", "JS", "3S"], None, None)                        # one completion
TURN_GHOST = ([["AH", "KD"], ["QS", "QC"]], ["2C", "7D", "9H", "JS"], ["AS", "AD"], None)
TURN_GHOST_TOP25 = ([["AH", "KD"], ["QS", "QC"]], ["2C", "7D", "9H", "JS"], ["AS", "AD"], TOP25)
THREE_LEVEL = ([["AH", "KD"], ["AS", "KC"], ["AD", "KH"]], ["2H", "7H", "9C", "JS"], None, None)   # 3 level seats; AC KS makes 4
# Nine hands and the opponent on a royal board.  The evaluator the project is pinned to counts every hole card of the flush
# suit as a further kicker, so a hand with a spade beats the board: the board plays for all ten seats only when nobody can
# hold one.  TEN_WAY keeps the opponent off the spades -- the ghost cards take 2S and 3S and the range allows twos and
# threes only (suited 32 left out); under the reference's law the second card dealt may be the one FOLLOWING the tested
# one, here 4C at the most, which the known hands leave in the deck -- and is a ten-way split on every outcome.
# ROYAL_OPEN leaves the opponent unrestricted: it wins outright with any spade and shares ten ways without one.
_NINE = [["5C", "6D"], ["5D", "6C"], ["5H", "6H"], ["7C", "8D"], ["7D", "8C"], ["7H", "8H"], ["9C", "TD"], ["9D", "TC"],
         ["9H", "TH"]]
TEN_WAY = (_NINE, ["TS", "JS", "QS", "KS", "AS"], ["2S", "3S"], ["22", "33", "32O"])
ROYAL_OPEN = (_NINE, ["TS", "JS", "QS", "KS", "AS"], None, None)
SMALL = [HU_RIVER, TURN_GHOST, TURN_GHOST_TOP25, THREE_LEVEL, TEN_WAY, ROYAL_OPEN]
SMALL_IDS = ["hu_river", "turn_ghost", "turn_ghost_top25", "three_level", "ten_way", "royal_open"]

FLOP_TOP25 = ([["AH", "KH"], ["QS", "QC"]], ["2C", "7D", "9H"], None, TOP25)                   # C(45, 2) = 990 completions
# 52 cards less hero, known hand and ghost cards: C(46, 5) completions of C(41, 2) candidate hands
PREFLOP = ([["AH", "KH"], ["QS", "QC"]], [], ["AS", "AD"], None)


def n_players(case):
    return len(case[0]) + 1


def records(case, random_opponent=True):
    """-> (mcq_query record [1], mcq_query_ext record [1]); random_opponent=False: the all-in record of the same hands."""
    hands, board, ghost, opp = case
    b = ids(board)
    q = npa.pack_queries([ids(hands[0])], [b + [255] * (5 - len(b))], len(hands) + (1 if random_opponent else 0), 1)
    ext = npa.pack_query_ext(1, ghost=ids(ghost) if ghost else None, known=[ids(h) for h in hands[1:]],
                             opp_range=npa.range_bits(opp) if opp is not None else None)
    return q, ext


def rotated(case, s):
    """The case with hand s in the hero's seat."""
    hands, board, ghost, opp = case
    return ([hands[s]] + hands[:s] + hands[s + 1:], board, ghost, opp)


def batch(cases, random_opponent=True):
    recs = [records(c, random_opponent) for c in cases]
    return np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])


def words(row):
    return [int(x) for x in np.asarray(row).view(np.uint64).reshape(32)]


_host = {}


def host_row(case_key, case, law):
    """The host lane build's 32-word row of a case (cached: computed once, shared by the tests)."""
    from tests import hostsim_exact_seats as H
    key = (case_key, law)
    if key not in _host:
        _host[key] = H.exact(*records(case), law)
    return _host[key]
