"""Test-only host build of mcq_iteration_sum with the instantiation named by the caller (see hs_join.cpp)."""
import ctypes as C
import functools

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_join/hs_join.cpp")
    L.hs_join_run.restype = C.c_int
    L.hs_join_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def rows(queries, seed, first_qid, nopp, ndeal, uniform=False, ways=False):
    """Query i (16-byte records) with id first_qid + i through mcq_iteration_sum<.., nopp, ndeal, ..>: -> uint64 [n, 13 or 22]."""
    return hostbuild.rows(lib().hs_join_run, queries, 22 if ways else 13, seed, first_qid, nopp, ndeal, int(uniform), int(ways),
                          qid_at=1)
