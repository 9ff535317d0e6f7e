"""Test-only host build of the paired count of the dealing in epochs, both settings of its switch (see hs_paired.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

FULLREG = 9                   # MCQ_DEAL_FULLREG
RULES = (1, 2, 3, FULLREG)
BIAS = 0x40404040             # MCQ_HOLE_BIAS


@functools.cache
def lib():
    L = hostbuild.load("hostsim_paired/hs_paired.cpp")
    L.hs_paired_default.restype = C.c_int
    L.hs_paired_count2.restype = None
    L.hs_paired_count2.argtypes = [C.c_uint64] + [C.c_void_p] * 5
    L.hs_paired_plan.restype = C.c_int
    L.hs_paired_plan.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.hs_paired_positions.restype = C.c_int
    L.hs_paired_positions.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.hs_paired_run.restype = C.c_int
    L.hs_paired_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.hs_paired_replay.restype = C.c_int
    L.hs_paired_replay.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def shipped_switch():
    return lib().hs_paired_default()


def count2(pb, h0, h1b):
    """uint32 arrays -> (what mcq_hole_count2 adds, what two mcq_hole_count add with the bias taken off the second)"""
    pb, h0, h1b = (np.ascontiguousarray(a, np.uint32) for a in (pb, h0, h1b))
    assert pb.shape == h0.shape == h1b.shape and pb.ndim == 1
    out, single = np.zeros_like(pb), np.zeros_like(pb)
    lib().hs_paired_count2(len(pb), *(a.ctypes.data_as(C.c_void_p) for a in (pb, h0, h1b, out, single)))
    return out, single


def plan(n_plan, rule):
    """-> dict(cost, cost_paired, regs: per register 0 plain / 1 biased by its pair draw / 2 biased by its first scan,
    holes: per epoch) of the plan of n_plan draws"""
    out = np.zeros(15, np.int32)
    rc = lib().hs_paired_plan(n_plan, rule, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("hs_paired_plan: %d (%d draws, rule %d)" % (rc, n_plan, rule))
    return {"cost": int(out[1]), "cost_paired": int(out[2]), "regs": [int(v) for v in out[3:9]],
            "holes": [int(v) for v in out[9:9 + int(out[0])]]}


def positions(n_plan, rule, draws, paired=True):
    """draws uint8 [rows, n], n <= n_plan: the first n draws of the plan -> base positions uint8 [rows, n]"""
    d = np.ascontiguousarray(draws, np.uint8)
    pos = np.full(d.shape, 255, np.uint8)
    rc = lib().hs_paired_positions(n_plan, rule, int(paired), d.shape[1], d.ctypes.data_as(C.c_void_p), d.shape[0],
                                   pos.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("hs_paired_positions: %d (%d draws of %d, rule %d)" % (rc, d.shape[1], n_plan, rule))
    return pos


def rows(queries, seed, first_qid, nopp, ndeal, uniform=False, ways=False, paired=True):
    """Query i (16-byte records) with id first_qid + i through mcq_iteration_sum<.., nopp, ndeal, ..>: -> uint64 [n, 13 or 22]."""
    return hostbuild.rows(lib().hs_paired_run, queries, 22 if ways else 13, seed, first_qid, nopp, ndeal, int(uniform), int(ways),
                          int(paired), qid_at=1)


def replay_rows(queries, seed32):
    """Parity mode: query i from the start of the MT19937 stream of seed32 -> uint64 [n, 13]."""
    return hostbuild.rows(lib().hs_paired_replay, queries, 13, seed32)
