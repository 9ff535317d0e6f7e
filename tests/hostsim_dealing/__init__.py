"""Test-only host build of the dealing's single-hole step and of the iteration with counted draws (see hs_dealing.cpp)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_dealing.so")
_SRCS = [os.path.join(_HERE, "hs_dealing.cpp"), os.path.join(_CSRC, "mcq_device.hpp"),
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
        L.hs_dealing_step.restype = C.c_int
        L.hs_dealing_step.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.hs_dealing_run.restype = C.c_int
        L.hs_dealing_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib
