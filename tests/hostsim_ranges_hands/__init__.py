"""Test-only host build of the per-hand entry of the weighted-range-per-seat Monte-Carlo path (see hs_ranges_hands.cpp):
the lane code with the per-hand accumulator and the block tally of mcq_hands.hpp, in the kernel's block / round / wave
order."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

FAILED = 2   # hs_ranges_hands_run: the failure marker (an iteration without an accepted trial)


@functools.cache
def lib():
    L = hostbuild.load("hostsim_ranges_hands/hs_ranges_hands.cpp")
    L.hs_ranges_hands_run.restype = C.c_int
    L.hs_hands_drive.restype = C.c_uint32
    L.hs_hands_increment.restype = C.c_uint32
    return L


def run_batch(queries, seat_table, tables, seed, first_qid, seat, grid=1, waves=16, trials=None, flushes=False):
    """n records on `grid` blocks of `waves` waves -> (rows uint64 [n, 32], hands uint64 [n, 1326, 4]) (and, with
    flushes=True, the number of flushes in the middle of a record's piece).  seat_table: [n, <= 10] table numbers, tables:
    uint16 [n_tables, 1326], trials: the records' prices (default 1).  ValueError(-1) for what the library refuses before
    a launch, ValueError(FAILED) for the failure marker."""
    q = np.ascontiguousarray(queries).view(np.uint8).reshape(-1, 16).copy()
    n = len(q)
    st = np.zeros((n, 10), np.uint32)
    seat_table = np.asarray(seat_table, np.uint32).reshape(n, -1)
    st[:, :seat_table.shape[1]] = seat_table
    tb = np.ascontiguousarray(tables, np.uint16).reshape(-1, 1326)
    tr = np.ones(n, np.uint32) if trials is None else np.ascontiguousarray(trials, np.uint32).reshape(n)
    out = np.zeros((n, 32), np.uint64)
    hands = np.zeros((n, 1326, 4), np.uint64)
    fl = C.c_uint32(0)
    rc = lib().hs_ranges_hands_run(q.ctypes.data_as(C.c_void_p), C.c_uint32(n), st.ctypes.data_as(C.c_void_p),
                                   tb.ctypes.data_as(C.c_void_p), C.c_uint32(len(tb)), tr.ctypes.data_as(C.c_void_p),
                                   C.c_uint64(seed), C.c_uint64(first_qid), C.c_uint32(seat), C.c_uint32(grid), C.c_uint32(waves),
                                   out.ctypes.data_as(C.c_void_p), hands.ctypes.data_as(C.c_void_p), C.byref(fl))
    if rc:
        raise ValueError(rc)
    return (out, hands, fl.value) if flushes else (out, hands)


def run(query16, seat_table, tables, seed, qid, seat, **kw):
    """One record -> (row uint64 [32], hands uint64 [1326, 4])."""
    res = run_batch(hostbuild.first_bytes(query16, 16), np.asarray(seat_table, np.uint32).reshape(1, -1), tables, seed, qid,
                    seat, **kw)
    return (res[0][0], res[1][0]) + tuple(res[2:])


def constants():
    """-> dict of mcq_hands.hpp's constants"""
    out = np.zeros(4, np.uint32)
    lib().hs_hands_constants(out.ctypes.data_as(C.c_void_p))
    return dict(zip(("table_words", "round_iters", "flush_rounds", "share_unit"), (int(x) for x in out)))


def increment(k):
    """mcq_seat_increment's word for k hands level"""
    return int(lib().hs_hands_increment(C.c_uint32(k)))


def drive(a, b, inc, n_adds, with_flush):
    """The hand (a, b) takes `inc` n_adds times, in rounds, the table flushed by the kernel's rule or only at the end
    -> (the hand's row [4] as ints, flushes before the end, words of other hands that are not zero)."""
    row = np.zeros(4, np.uint64)
    other = C.c_uint32(0)
    fl = lib().hs_hands_drive(C.c_uint32(a), C.c_uint32(b), C.c_uint32(inc), C.c_uint64(n_adds), C.c_int(int(with_flush)),
                              row.ctypes.data_as(C.c_void_p), C.byref(other))
    return [int(x) for x in row], int(fl), int(other.value)


def piece(pfx, weight, n_tasks, blo, bhi, waves=16):
    """-> (first, end, rounds) of a record's tasks in a block's piece of the cost axis"""
    out = np.zeros(3, np.uint32)
    lib().hs_hands_piece(C.c_uint64(pfx), C.c_uint32(weight), C.c_uint32(n_tasks), C.c_uint64(blo), C.c_uint64(bhi),
                         C.c_uint32(waves), out.ctypes.data_as(C.c_void_p))
    return tuple(int(x) for x in out)
