"""Test-only host build of the table-card position arithmetic and the deck accessors (see hs_deck.cpp)."""
import ctypes as C
import functools

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_deck/hs_deck.cpp")
    L.hs_deck_both.restype = C.c_int64
    return L
