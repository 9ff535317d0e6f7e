"""Test-only host build of the opponents' cards read by flush suit (see hs_bysuit.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

POSITIONS = 50
# accessors of hs_bysuit_run
DEALT, BY_SUIT_CARDS, BY_SUIT_POSITION_MAJOR, BY_SUIT_SUIT_MAJOR = 0, 1, 2, 3
# sources of hs_bysuit_entries
ENTRY_SOURCES = ("set + perm", "array of cards", "arrays of halves", "position-major table", "suit-major table")


@functools.cache
def lib():
    L = hostbuild.load("hostsim_bysuit/hs_bysuit.cpp")
    L.hs_bysuit_default.restype = C.c_int
    L.hs_bysuit_rank_weight2.restype = C.c_uint32
    L.hs_bysuit_rank_weight2.argtypes = [C.c_uint32]
    L.hs_bysuit_wave_bytes.restype = C.c_uint32
    L.hs_bysuit_entries.restype = C.c_int
    L.hs_bysuit_entries.argtypes = [C.c_void_p, C.c_void_p]
    L.hs_bysuit_run.restype = C.c_int
    L.hs_bysuit_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def shipped():
    """whether the product's straight forms read the opponents' cards by suit"""
    return bool(lib().hs_bysuit_default())


def rank_weight2(rank):
    return int(lib().hs_bysuit_rank_weight2(rank))


def wave_bytes():
    return int(lib().hs_bysuit_wave_bytes())


def entries(query):
    """one 16-byte query record -> (deck length, uint32 [5 sources, 50 positions, 4 suits, 2 words])"""
    rec = np.ascontiguousarray(query).view(np.uint8).reshape(16).copy()
    out = np.full((len(ENTRY_SOURCES), POSITIONS, 4, 2), 0xEEEEEEEE, np.uint32)
    rc = lib().hs_bysuit_entries(rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise ValueError("hs_bysuit_entries: %d (query %s)" % (rc, rec.tolist()))
    return rc, out


def rows(queries, seed, first_qid, nopp, ndeal, accessor, uniform=False, ways=False):
    """Query i (16-byte records) with id first_qid + i through mcq_iteration_sum<.., nopp, ndeal, ..> -> uint64 [n, 13 or 22]."""
    return hostbuild.rows(lib().hs_bysuit_run, queries, 22 if ways else 13, seed, first_qid, nopp, ndeal, int(uniform), int(ways),
                          accessor, qid_at=1)
