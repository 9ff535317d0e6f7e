"""Test-only host build of the exact per-seat lane code with one random opponent (see hs_exact_seats.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

REFUSALS = {1: "invalid", 2: "hero range", 3: "known range", 4: "too many random opponents", 5: "range cannot be dealt",
            6: "two random opponents"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_exact_seats/hs_exact_seats.cpp")
    L.hs_exact_ext_seats.restype = C.c_int
    return L


def exact(query16, ext304, law):
    """One record through the per-seat lane code -> the 32 words of its mcq_result_seats row of integer weights (law: 0
    reference, 1 uniform).  ValueError(reason) on a refusal."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(32, np.uint64)
    rc = lib().hs_exact_ext_seats(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(law),
                                  out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(REFUSALS.get(rc, rc))
    return out
