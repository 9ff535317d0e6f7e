"""Test-only host build of mcq_iteration_sum with the instantiation named by the caller (see hs_join.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_join/hs_join.cpp")
    L.hs_join_run.restype = C.c_int
    L.hs_join_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def rows(queries, seed, first_qid, nopp, ndeal, uniform=False, ways=False):
    """Query i (16-byte records) with id first_qid + i through mcq_iteration_sum<.., nopp, ndeal, ..>: -> uint64 [n, 13 or 22]."""
    L = lib()
    q = np.ascontiguousarray(queries).view(np.uint8).reshape(-1, 16)
    out = np.zeros((len(q), 22 if ways else 13), np.uint64)
    for i in range(len(q)):
        rec = q[i].copy()
        rc = L.hs_join_run(rec.ctypes.data_as(C.c_void_p), seed, first_qid + i, nopp, ndeal, int(uniform), int(ways),
                           out[i].ctypes.data_as(C.c_void_p))
        if rc:
            raise ValueError("hs_join_run: %d (nopp %d, ndeal %d, query %s)" % (rc, nopp, ndeal, rec.tolist()))
    return out
