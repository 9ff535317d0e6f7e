"""Test-only host build of the extended lane code with the per-seat switch on (see hs_seats.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_seats/hs_seats.cpp")
    L.hs_seats_run.restype = C.c_int
    L.hs_seats_exact.restype = C.c_int
    return L


def run(query16, ext304, seed, qid, hands=False):
    """One extended query through the per-seat lane code (MCQ-CTR v5x streams of (seed, qid)) -> the 32 words of its
    mcq_result_seats row (and, with hands=True, every iteration's dealt hands: [runs, 2 * n_players + 5] card ids, the five
    table cards last).  ValueError(code) for what the library refuses (an invalid record, an undealable range)."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(32, np.uint64)
    runs, n_players = int(q[12:16].view("<u4")[0]), int(q[8])
    tr = np.full((max(runs, 1), 2 * n_players + 5), 255, np.uint8) if hands else None
    rc = lib().hs_seats_run(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_uint64(seed), C.c_uint64(qid),
                            out.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p) if hands else None)
    if rc:
        raise ValueError(rc)
    return (out, tr[:runs]) if hands else out


def exact_refusal(query16, ext304, law):
    """Why the all-in enumeration refuses a record: 0 = it does not, 1..4 = MCQ_XX_* (invalid, hero range, ranged known
    hand, too many random opponents), 5 = cannot be dealt, 7 = a random opponent."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(32, np.uint64)
    return int(lib().hs_seats_exact(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(law),
                                    out.ctypes.data_as(C.c_void_p)))


def exact(query16, ext304, law):
    """The all-in enumeration's per-seat lane code -> 32 words of integer weights; ValueError(code) on a refusal."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(32, np.uint64)
    rc = lib().hs_seats_exact(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(law),
                              out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(rc)
    return out
