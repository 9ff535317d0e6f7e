"""Test-only host build of the hand-against-hand matrix's lane code (see hs_matrix.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_matrix.so")
_SRCS = [os.path.join(_HERE, "hs_matrix.cpp"), os.path.join(_CSRC, "mcq_device.hpp"), os.path.join(_CSRC, "mcq_exact.hpp"),
         os.path.join(_CSRC, "mcq_exact_ext.hpp"), os.path.join(_CSRC, "mcq_exact_hero.hpp"),
         os.path.join(_CSRC, "mcq_exact_matrix.hpp"), os.path.join(_HERE, "..", "..", "include", "mcq.h")]
_lib = None

ROWS = 1326
SENTINEL = 0xA5A5
REFUSALS = {-2: "no win matrix", 1: "street", 2: "reserved bytes", 3: "mask bits", 4: "card out of range", 5: "table card twice",
            6: "table card dead", 7: "too few cards"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            tmp = _SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
                                   "-pthread", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.hs_matrix.restype = C.c_int
        L.hs_matrix.argtypes = [C.c_void_p] * 4
        _lib = L
    return _lib


def matrix(query16, want_tie=True, want_win=True):
    """-> (win[1326, 1326] uint16, tie[1326, 1326] uint16 or None, total).  A refusal raises ValueError after checking that
    it left the sentinel-filled outputs untouched."""
    q = np.ascontiguousarray(query16).view(np.uint8).reshape(-1)[:16].copy()
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
