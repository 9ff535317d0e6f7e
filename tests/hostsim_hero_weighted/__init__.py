"""Test-only host build of the weighted hero-range exact enumeration's lane code (see hs_hero_weighted.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

ROWS = 1326
SENTINEL = 0xA5A5A5A5A5A5A5A5
REFUSALS = {-2: "no opponent weights", 1: "invalid", 2: "hero is not a range", 3: "known hands", 4: "not heads-up", 5: "preflop",
            6: "no allowed hero hand", 7: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_hero_weighted/hs_hero_weighted.cpp")
    L.hs_hero_weighted.restype = C.c_int
    L.hs_hero_weighted.argtypes = [C.c_void_p] * 6
    return L


def _table(w, name):
    if w is None:
        return None
    w = np.ascontiguousarray(w)
    if w.dtype != np.uint16 or w.size != ROWS:
        raise TypeError("%s: %d uint16 weights" % (name, ROWS))
    return w.reshape(ROWS).copy()


def hero_weighted(query16, ext, opp_w, hero_w=None):
    """-> (rows[1326, 13] uint64 like result rows, agg[11] float64: win, tie, by_type[9]).  A refusal raises ValueError
    after checking that it left both outputs untouched."""
    q, e = hostbuild.record(query16, ext)
    ow, hw = _table(opp_w, "opp_w"), _table(hero_w, "hero_w")
    rows = np.full((ROWS, 13), SENTINEL, np.uint64)
    agg = np.full(11, -7.0, np.float64)
    rc = lib().hs_hero_weighted(q.ctypes.data, e.ctypes.data, None if ow is None else ow.ctypes.data,
                                None if hw is None else hw.ctypes.data, rows.ctypes.data, agg.ctypes.data)
    if rc:
        assert (rows == SENTINEL).all() and (agg == -7.0).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    return rows, agg
