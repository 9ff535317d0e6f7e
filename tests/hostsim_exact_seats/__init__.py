"""Test-only host build of the exact per-seat lane code with one random opponent (see hs_exact_seats.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_exact_seats.so")
_SRCS = [os.path.join(_HERE, "hs_exact_seats.cpp"), os.path.join(_CSRC, "mcq_device.hpp"), os.path.join(_CSRC, "mcq_exact.hpp"),
         os.path.join(_CSRC, "mcq_exact_ext.hpp"), os.path.join(_HERE, "..", "..", "include", "mcq.h")]
_lib = None

REFUSALS = {1: "invalid", 2: "hero range", 3: "known range", 4: "too many random opponents", 5: "range cannot be dealt",
            6: "two random opponents"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            tmp = _SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
                                   "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.hs_exact_ext_seats.restype = C.c_int
        _lib = L
    return _lib


def exact(query16, ext304, law):
    """One record through the per-seat lane code -> the 32 words of its mcq_result_seats row of integer weights (law: 0
    reference, 1 uniform).  ValueError(reason) on a refusal."""
    q = np.ascontiguousarray(query16).view(np.uint8).reshape(-1)[:16].copy()
    e = np.ascontiguousarray(ext304).view(np.uint8).reshape(-1)[:304].copy()
    out = np.zeros(32, np.uint64)
    rc = lib().hs_exact_ext_seats(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(law),
                                  out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(REFUSALS.get(rc, rc))
    return out
