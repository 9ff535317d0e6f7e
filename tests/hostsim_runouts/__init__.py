"""Test-only host build of the per-runout exact enumeration's lane code (see hs_runouts.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

CARD_ROWS, PAIR_ROWS, WORDS = 52, 1326, 22
SENTINEL = 0xA5A5A5A5A5A5A5A5
REFUSALS = {-1: "bad law", 1: "invalid", 2: "hero range", 3: "ranged known hand", 4: "too many opponents",
            5: "two random opponents", 6: "preflop", 7: "river", 8: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_runouts/hs_runouts.cpp")
    L.hs_runouts.restype = C.c_int
    return L


def runouts(query16, ext, law=0):
    """-> (cards[52, 22], pairs[1326, 22]) uint64 like mcq_result_ways rows.  A refusal raises ValueError after checking that
    it left both outputs untouched."""
    q, e = hostbuild.record(query16, ext)
    cards = np.full((CARD_ROWS, WORDS), SENTINEL, np.uint64)
    pairs = np.full((PAIR_ROWS, WORDS), SENTINEL, np.uint64)
    rc = lib().hs_runouts(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(int(law)),
                          cards.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p))
    if rc:
        assert (cards == SENTINEL).all() and (pairs == SENTINEL).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    return cards, pairs
