"""Test-only host build of the lane code with the split-pot switch on (see hs_ways.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_ways/hs_ways.cpp")
    L.hs_ways_run.restype = C.c_int
    L.hs_ways_row_bytes.restype = C.c_uint32
    return L


def run(mode, query16, seed, qid=0, general=False):
    """One query through the lane code -> the 22 words of its mcq_result_ways row.  mode: oracle.MODE_MT / MODE_CTR /
    MODE_CTR_UNIFORM; general=True: the general form of mcq_iteration (what the one-launch kernel runs)."""
    q = hostbuild.first_bytes(query16, 16)
    out = np.zeros(22, np.uint64)
    rc = lib().hs_ways_run(C.c_int(mode), q.ctypes.data_as(C.c_void_p), C.c_uint64(seed), C.c_uint64(qid),
                           C.c_int(1 if general else 0), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(rc)
    return out
