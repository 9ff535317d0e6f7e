"""Test-only host build of the dealing's single-hole step and of the iteration with counted draws (see hs_dealing.cpp)."""
import ctypes as C
import functools

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_dealing/hs_dealing.cpp")
    L.hs_dealing_step.restype = C.c_int
    L.hs_dealing_step.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.hs_dealing_run.restype = C.c_int
    L.hs_dealing_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L
