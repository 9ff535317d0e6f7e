"""Test-only host build of the plain path's iteration, folded into result rows (see hs_diet.cpp)."""
import ctypes as C
import functools

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_diet/hs_diet.cpp")
    L.hs_diet_run.restype = C.c_int
    L.hs_diet_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    L.hs_diet_card_sum.restype = C.c_uint32
    L.hs_diet_card_sum.argtypes = [C.c_uint32]
    L.hs_diet_psel.restype = C.c_uint32
    L.hs_diet_psel.argtypes = [C.c_void_p, C.c_uint32]
    return L
