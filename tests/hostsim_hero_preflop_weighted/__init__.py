"""Test-only host build of the weighted preflop hero-range exact enumeration's lane code (see hs_hero_preflop_weighted.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

ROWS = 1326
SENTINEL = 0xA5A5A5A5A5A5A5A5
REFUSALS = {-3: "no opponent weights", -2: "empty completion range", 1: "invalid", 2: "hero is not a range", 3: "known hands",
            4: "not heads-up", 6: "no allowed hero hand", 7: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_hero_preflop_weighted/hs_hero_preflop_weighted.cpp")
    L.hs_hero_pre_w.restype = C.c_int
    L.hs_hero_pre_w.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 2 + [C.c_void_p] * 3
    L.hs_hero_pre_w_allowed.restype = C.c_int
    L.hs_hero_pre_w_allowed.argtypes = [C.c_void_p] * 5
    L.hs_hero_pre_w_walked.restype = C.c_uint64
    L.hs_hero_pre_w_walked.argtypes = []
    return L


def _table(w, name):
    if w is None:
        return None
    w = np.ascontiguousarray(w)
    if w.dtype != np.uint16 or w.size != ROWS:
        raise TypeError("%s: %d uint16 weights" % (name, ROWS))
    return w.reshape(ROWS).copy()


def walked():
    """How many completions every call so far has ranked."""
    return int(lib().hs_hero_pre_w_walked())


def hero_pre_w(query16, ext, opp_w, hero_w=None, lo=0, hi=0xFFFFFFFF):
    """-> (rows[1326, 13] uint64: the partial rows of the completions [lo, hi), agg[11] float64 or None when the range does
    not cover every completion, counts: allowed, live, ranked, completions).  A refusal raises ValueError after checking that
    it left the outputs untouched."""
    q, e = hostbuild.record(query16, ext)
    ow, hw = _table(opp_w, "opp_w"), _table(hero_w, "hero_w")
    rows = np.full((ROWS, 13), SENTINEL, np.uint64)
    agg = np.full(11, -7.0, np.float64)
    counts = np.full(4, 0xFFFFFFFF, np.uint32)
    rc = lib().hs_hero_pre_w(q.ctypes.data, e.ctypes.data, None if ow is None else ow.ctypes.data,
                             None if hw is None else hw.ctypes.data, lo, hi, rows.ctypes.data, agg.ctypes.data, counts.ctypes.data)
    if rc:
        assert (rows == SENTINEL).all() and (agg == -7.0).all() and (counts == 0xFFFFFFFF).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    whole = lo == 0 and hi >= int(counts[3])
    assert whole == bool((agg != -7.0).any())
    return rows, (agg if whole else None), [int(v) for v in counts]


def allowed_rows(query16, ext, opp_w, hero_w=None):
    """The rows of the allowed hero hands in the order of the kernel's `allowed` list."""
    q, e = hostbuild.record(query16, ext)
    ow, hw = _table(opp_w, "opp_w"), _table(hero_w, "hero_w")
    out = np.zeros(ROWS, np.uint32)
    n = lib().hs_hero_pre_w_allowed(q.ctypes.data, e.ctypes.data, ow.ctypes.data, None if hw is None else hw.ctypes.data,
                                    out.ctypes.data)
    if n < 0:
        raise ValueError("refused")
    return [int(v) for v in out[:n]]
