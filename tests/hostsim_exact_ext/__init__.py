"""Test-only host build of the extended exact enumeration's lane code (see hs_exact_ext.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

REFUSALS = {1: "invalid", 2: "hero range", 3: "known range", 4: "too many random opponents", 5: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_exact_ext/hs_exact_ext.cpp")
    L.hs_exact_ext.restype = C.c_int
    L.hs_exact_ext_r.restype = C.c_int
    return L


def exact_ext(query16, ext, uniform=False):
    """-> (prob[11] float64: win, tie, by_type[9]; weights[13] uint64 like a result row).  A refusal raises ValueError."""
    q, e = hostbuild.record(query16, ext)
    prob = np.zeros(11, np.float64)
    w = np.zeros(13, np.uint64)
    rc = lib().hs_exact_ext(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(1 if uniform else 0),
                            prob.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(REFUSALS.get(rc, rc))
    return prob, w
