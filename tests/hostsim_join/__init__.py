"""Test-only host build of mcq_iteration_sum with the instantiation named by the caller (see hs_join.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_join.so")
_SRCS = [os.path.join(_HERE, "hs_join.cpp"), os.path.join(_CSRC, "mcq_device.hpp"),
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
        L.hs_join_run.restype = C.c_int
        L.hs_join_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


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
