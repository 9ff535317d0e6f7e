"""Test-only host build of the hero-range exact enumeration's lane code (see hs_hero_range.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

ROWS = 1326
REFUSALS = {-1: "bad law", 1: "invalid", 2: "hero is not a range", 3: "known hands", 4: "not heads-up", 5: "preflop",
            6: "no allowed hero hand", 7: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_hero_range/hs_hero_range.cpp")
    L.hs_hero_range.restype = C.c_int
    L.hs_hero_weights.restype = C.c_int
    return L


def hero_range(query16, ext, law=0):
    """-> (rows[1326, 13] uint64 like result rows, agg[11] float64: win, tie, by_type[9]).  A refusal raises ValueError
    after checking that it left both outputs untouched."""
    q, e = hostbuild.record(query16, ext)
    rows = np.full((ROWS, 13), 0xA5A5A5A5A5A5A5A5, np.uint64)
    agg = np.full(11, -7.0, np.float64)
    rc = lib().hs_hero_range(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(int(law)),
                             rows.ctypes.data_as(C.c_void_p), agg.ctypes.data_as(C.c_void_p))
    if rc:
        assert (rows == 0xA5A5A5A5A5A5A5A5).all() and (agg == -7.0).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    return rows, agg


def hero_weights(query16, ext, law=0):
    """-> w[1326] uint32: how often the law deals hero each hand, in proportion (0 = not an allowed hand of the deck)."""
    q, e = hostbuild.record(query16, ext)
    w = np.zeros(ROWS, np.uint32)
    rc = lib().hs_hero_weights(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(int(law)),
                               w.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise ValueError("refused")
    return w
