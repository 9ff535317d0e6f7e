"""Test-only host build of the lane code of the weighted-range-per-seat Monte-Carlo entry (see hs_ranges.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

FAILED = 2   # hs_ranges_run: the failure marker (an iteration without an accepted trial)


@functools.cache
def lib():
    L = hostbuild.load("hostsim_ranges/hs_ranges.cpp")
    L.hs_ranges_run.restype = C.c_int
    L.hs_ranges_pick.restype = C.c_uint32
    return L


def run(query16, seat_table, tables, seed, qid, hands=False):
    """One record through the lane code (streams of (seed, qid), tasks and lanes one behind the other) -> the 32 words of
    its mcq_result_seats row (and, with hands=True, every iteration's deal: [runs, 2 * n_players + 5] card ids, the five
    table cards last).  seat_table: ten table numbers, tables: uint16 [n_tables, 1326].
    ValueError(-1) for what the library refuses before a launch, ValueError(FAILED) for the failure marker."""
    q = hostbuild.first_bytes(query16, 16)
    st = np.zeros(10, np.uint32)
    seat_table = np.asarray(seat_table, np.uint32).reshape(-1)
    st[:len(seat_table)] = seat_table
    tb = np.ascontiguousarray(tables, np.uint16).reshape(-1, 1326)
    out = np.zeros(32, np.uint64)
    runs, n_players = int(q[12:16].view("<u4")[0]), int(q[8])
    tr = np.full((max(runs, 1), 2 * n_players + 5), 255, np.uint8) if hands else None
    rc = lib().hs_ranges_run(q.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p),
                             C.c_uint32(len(tb)), C.c_uint64(seed), C.c_uint64(qid), out.ctypes.data_as(C.c_void_p),
                             tr.ctypes.data_as(C.c_void_p) if hands else None)
    if rc:
        raise ValueError(rc)
    return (out, tr[:runs]) if hands else out


def pick(table, word):
    """The hand (a, b), a < b, that draw word `word` selects from one uint16 [1326] table."""
    tb = np.ascontiguousarray(table, np.uint16).reshape(1326)
    v = int(lib().hs_ranges_pick(tb.ctypes.data_as(C.c_void_p), C.c_uint32(word)))
    return v & 0xFF, v >> 8
