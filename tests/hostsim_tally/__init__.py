"""Test-only host build of the wave tallies (neuron_poker_amd/csrc/mcq_tally.hpp; see hs_tally.cpp): the fold of lane
accumulators into a row and the lane states' lanes -> row step for a simulated wave of 64 lanes.

An accumulator travels as a record of REC 64-bit words: plain (types, tie, passes), split-pot (types, passes, ways),
per-seat (passes, seat[0..9])."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

PLAIN, WAYS, SEATS = 0, 1, 2
WAVE, REC, ROW = 64, 12, 32
_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@functools.cache
def lib():
    L = hostbuild.load("hostsim_tally/hs_tally.cpp")
    u32 = C.c_uint32
    L.hs_tally_consts.argtypes = [_U32P]
    L.hs_tally_consts.restype = None
    L.hs_tally_fold.argtypes = [u32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.hs_tally_wave.argtypes = [u32, u32, C.c_void_p, u32, C.c_void_p]
    L.hs_tally_ways_state.argtypes = [C.c_void_p, u32, _U32P]
    L.hs_tally_ways_state.restype = None
    L.hs_tally_seats_flush.argtypes = [C.c_void_p, u32, C.c_void_p, _U32P]
    L.hs_tally_clear_is_clean.argtypes = [u32, C.c_void_p, u32]
    return L


@functools.cache
def consts():
    out = (C.c_uint32 * 11)()
    lib().hs_tally_consts(out)
    names = ("plain_words", "plain_lanes", "ways_words", "ways_lanes", "seats_words", "seats_lanes", "ways_tally_tasks",
             "direct_tasks_limit", "n_codes", "n_ways", "max_seats")
    return dict(zip(names, (int(x) for x in out)))


def _recs(recs, *shape):
    r = np.ascontiguousarray(recs, np.uint64)
    assert r.shape[-len(shape):] == shape, r.shape
    return r


def fold(kind, recs):
    """records [n][REC] -> the ROW words of a zero row they fold into"""
    r = _recs(recs, REC).reshape(-1, REC)
    row = np.zeros(ROW, np.uint64)
    assert lib().hs_tally_fold(kind, r.ctypes.data, len(r), row.ctypes.data) == 0
    return row


def wave(kind, recs, packed=False):
    """records [tasks][WAVE][REC] added to a cleared wave -> the word each of the WAVE lanes holds after the row step"""
    r = _recs(recs, WAVE, REC)
    words = np.zeros(WAVE, np.uint64)
    assert lib().hs_tally_wave(kind, int(packed), r.ctypes.data, len(r), words.ctypes.data) == 0
    return words


def ways_state(recs):
    """split-pot records [tasks][REC] added to one cleared lane, no flush -> (way3[3], n_add, full, way[9])"""
    r = _recs(recs, REC)
    out = (C.c_uint32 * 14)()
    lib().hs_tally_ways_state(r.ctypes.data, len(r), out)
    v = [int(x) for x in out]
    return v[:3], v[3], bool(v[4]), v[5:]


def seats_flush(recs):
    """per-seat records [tasks][WAVE][REC] -> (row, atomics of a clean wave's flush, of the flush after the tasks, of a
    second flush, every lane clear after the flush)"""
    r = _recs(recs, WAVE, REC)
    row = np.zeros(ROW, np.uint64)
    out = (C.c_uint32 * 4)()
    assert lib().hs_tally_seats_flush(r.ctypes.data, len(r), row.ctypes.data, out) == 0
    return row, int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def clear_is_clean(kind, recs):
    r = _recs(recs, WAVE, REC)
    return lib().hs_tally_clear_is_clean(kind, r.ctypes.data, len(r)) == 1
