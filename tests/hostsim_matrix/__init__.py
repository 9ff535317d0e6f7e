"""Test-only host build of the hand-against-hand matrix's lane code (see hs_matrix.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

ROWS = 1326
SENTINEL = 0xA5A5
REFUSALS = {-2: "no win matrix", 1: "street", 2: "reserved bytes", 3: "mask bits", 4: "card out of range", 5: "table card twice",
            6: "table card dead", 7: "too few cards"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_matrix/hs_matrix.cpp")
    L.hs_matrix.restype = C.c_int
    L.hs_matrix.argtypes = [C.c_void_p] * 4
    return L


def matrix(query16, want_tie=True, want_win=True):
    """-> (win[1326, 1326] uint16, tie[1326, 1326] uint16 or None, total).  A refusal raises ValueError after checking that
    it left the sentinel-filled outputs untouched."""
    q = hostbuild.first_bytes(query16, 16)
    win = np.full((ROWS, ROWS), SENTINEL, np.uint16)
    tie = np.full((ROWS, ROWS), SENTINEL, np.uint16)
    total = np.full(1, 0xA5A5A5A5, np.uint32)
    rc = lib().hs_matrix(q.ctypes.data, win.ctypes.data if want_win else None, tie.ctypes.data if want_tie else None,
                         total.ctypes.data)
    if rc:
        assert (win == SENTINEL).all() and (tie == SENTINEL).all() and total[0] == 0xA5A5A5A5, "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    if not want_tie:
        assert (tie == SENTINEL).all()
    return win, (tie if want_tie else None), int(total[0])
