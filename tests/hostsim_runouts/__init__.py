"""Test-only host build of the per-runout exact enumeration's lane code (see hs_runouts.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_runouts.so")
_SRCS = [os.path.join(_HERE, "hs_runouts.cpp"), os.path.join(_CSRC, "mcq_device.hpp"), os.path.join(_CSRC, "mcq_exact.hpp"),
         os.path.join(_CSRC, "mcq_exact_ext.hpp"), os.path.join(_CSRC, "mcq_exact_runout.hpp"),
         os.path.join(_HERE, "..", "..", "include", "mcq.h")]
_lib = None

CARD_ROWS, PAIR_ROWS, WORDS = 52, 1326, 22
SENTINEL = 0xA5A5A5A5A5A5A5A5
REFUSALS = {-1: "bad law", 1: "invalid", 2: "hero range", 3: "ranged known hand", 4: "too many opponents",
            5: "two random opponents", 6: "preflop", 7: "river", 8: "range cannot be dealt"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            tmp = _SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
                                   "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.hs_runouts.restype = C.c_int
        _lib = L
    return _lib


def runouts(query16, ext, law=0):
    """-> (cards[52, 22], pairs[1326, 22]) uint64 like mcq_result_ways rows.  A refusal raises ValueError after checking that
    it left both outputs untouched."""
    q = np.ascontiguousarray(query16).view(np.uint8).reshape(-1)[:16].copy()
    e = np.ascontiguousarray(ext).view(np.uint8).reshape(-1)[:304].copy()
    cards = np.full((CARD_ROWS, WORDS), SENTINEL, np.uint64)
    pairs = np.full((PAIR_ROWS, WORDS), SENTINEL, np.uint64)
    rc = lib().hs_runouts(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(int(law)),
                          cards.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p))
    if rc:
        assert (cards == SENTINEL).all() and (pairs == SENTINEL).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    return cards, pairs
