"""Test-only host build of the table-card position arithmetic and the deck accessors (see hs_deck.cpp)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_deck.so")
_SRCS = [os.path.join(_HERE, "hs_deck.cpp"), os.path.join(_CSRC, "mcq_device.hpp"),
         os.path.join(_HERE, "..", "..", "include", "mcq.h")]
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            tmp = _SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
                                   "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.hs_deck_both.restype = C.c_int64
        _lib = L
    return _lib
