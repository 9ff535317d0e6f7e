"""Test-only host build of the sum-form evaluator (see hs_sum.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

N_CODES = 10


@functools.cache
def lib():
    L = hostbuild.load("hostsim_sum/hs_sum.cpp")
    L.hs_sum_multisets.restype = C.c_uint32
    L.hs_sum_sweep.restype = C.c_uint64
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def info():
    """-> dict: rows, slots, shift, image_bytes, fits, ids_by_code"""
    out = np.zeros(5 + N_CODES, np.uint32)
    lib().hs_sum_info(_p(out))
    return {"rows": int(out[0]), "slots": int(out[1]), "shift": int(out[2]), "image_bytes": int(out[3]),
            "fits": bool(out[4]), "ids_by_code": [int(v) for v in out[5:]]}


def tables():
    """-> hoff, hrank, tfid, tf (the mask form's flush table, keys)"""
    i = info()
    hoff, hrank = np.zeros(i["rows"], np.uint16), np.zeros(i["slots"], np.uint16)
    tfid, tf = np.zeros(8192, np.uint32), np.zeros(8192, np.uint32)
    lib().hs_sum_tables(_p(hoff), _p(hrank), _p(tfid), _p(tf))
    return hoff, hrank, tfid, tf


def weights():
    w = np.zeros(13, np.uint32)
    lib().hs_sum_weights(_p(w))
    return w


def multisets():
    """-> sums, keys of every rank multiset"""
    sums, keys = np.zeros(65536, np.uint32), np.zeros(65536, np.uint32)
    n = lib().hs_sum_multisets(_p(sums), _p(keys))
    assert n <= 65536
    return sums[:n].copy(), keys[:n].copy()


def sweep(threads=8, stride=1, phase=0):
    """-> hands seen, hands that broke the id -> key map or the type, key_of_id[65536]"""
    m = np.zeros(65536, np.uint32)
    bad = C.c_uint64(0)
    n = lib().hs_sum_sweep(C.c_uint32(threads), C.c_uint32(stride), C.c_uint32(phase), _p(m), C.byref(bad))
    return int(n), int(bad.value), m
