"""Test-only host build of the opponents' cards read by flush suit (see hs_bysuit.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "neuron_poker_amd", "csrc")
_SO = os.path.join(_HERE, "libhs_bysuit.so")
_SRCS = [os.path.join(_HERE, "hs_bysuit.cpp"), os.path.join(_CSRC, "mcq_device.hpp"),
         os.path.join(_HERE, "..", "..", "include", "mcq.h")]
_lib = None

POSITIONS = 50
# accessors of hs_bysuit_run
DEALT, BY_SUIT_CARDS, BY_SUIT_POSITION_MAJOR, BY_SUIT_SUIT_MAJOR = 0, 1, 2, 3
# sources of hs_bysuit_entries
ENTRY_SOURCES = ("set + perm", "array of cards", "arrays of halves", "position-major table", "suit-major table")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            tmp = _SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
                                   "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.hs_bysuit_default.restype = C.c_int
        L.hs_bysuit_rank_weight2.restype = C.c_uint32
        L.hs_bysuit_rank_weight2.argtypes = [C.c_uint32]
        L.hs_bysuit_wave_bytes.restype = C.c_uint32
        L.hs_bysuit_entries.restype = C.c_int
        L.hs_bysuit_entries.argtypes = [C.c_void_p, C.c_void_p]
        L.hs_bysuit_run.restype = C.c_int
        L.hs_bysuit_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


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
    L = lib()
    q = np.ascontiguousarray(queries).view(np.uint8).reshape(-1, 16)
    out = np.zeros((len(q), 22 if ways else 13), np.uint64)
    for i in range(len(q)):
        rec = q[i].copy()
        rc = L.hs_bysuit_run(rec.ctypes.data_as(C.c_void_p), seed, first_qid + i, nopp, ndeal, int(uniform), int(ways),
                             accessor, out[i].ctypes.data_as(C.c_void_p))
        if rc:
            raise ValueError("hs_bysuit_run: %d (nopp %d, ndeal %d, accessor %d, query %s)" % (rc, nopp, ndeal, accessor, rec.tolist()))
    return out
