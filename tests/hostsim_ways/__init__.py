"""Test-only host build of the lane code with the split-pot switch on (see hs_ways.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_ways.so")
_SRCS = [os.path.join(_HERE, "hs_ways.cpp"), os.path.join(_CSRC, "mcq_device.hpp"), os.path.join(_CSRC, "mcq_replay.hpp"),
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
        L.hs_ways_run.restype = C.c_int
        L.hs_ways_row_bytes.restype = C.c_uint32
        _lib = L
    return _lib


def run(mode, query16, seed, qid=0, general=False):
    """One query through the lane code -> the 22 words of its mcq_result_ways row.  mode: oracle.MODE_MT / MODE_CTR /
    MODE_CTR_UNIFORM; general=True: the general form of mcq_iteration (what the one-launch kernel runs)."""
    q = np.ascontiguousarray(query16).view(np.uint8).reshape(-1)[:16].copy()
    out = np.zeros(22, np.uint64)
    rc = lib().hs_ways_run(C.c_int(mode), q.ctypes.data_as(C.c_void_p), C.c_uint64(seed), C.c_uint64(qid),
                           C.c_int(1 if general else 0), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(rc)
    return out
