"""Test-only host build of the dealing in epochs and of the iterations that deal by it (see hs_epochs.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

FULLREG = 9                   # MCQ_DEAL_FULLREG
RULES = (1, 2, 3, FULLREG)    # the plans built: at most one, two, three checkpoints; every full register


@functools.cache
def lib():
    L = hostbuild.load("hostsim_epochs/hs_epochs.cpp")
    L.hs_epochs_rule.restype = C.c_int
    L.hs_epochs_plan.restype = C.c_int
    L.hs_epochs_plan.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.hs_epochs_positions.restype = C.c_int
    L.hs_epochs_positions.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.hs_epochs_run.restype = C.c_int
    L.hs_epochs_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.hs_epochs_replay.restype = C.c_int
    L.hs_epochs_replay.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def shipped_rule():
    return lib().hs_epochs_rule()


def plan(n_plan, rule):
    """-> dict(checkpoints, reg0 (first register of every epoch, then the total), cost, valid) of the plan of n_plan draws"""
    out = np.zeros(17, np.int32)
    rc = lib().hs_epochs_plan(n_plan, rule, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("hs_epochs_plan: %d (%d draws, rule %d)" % (rc, n_plan, rule))
    ne = int(out[0])
    return {"checkpoints": [int(v) for v in out[2:1 + ne]], "reg0": [int(v) for v in out[8:9 + ne]], "cost": int(out[15]),
            "valid": bool(out[16])}


def positions(n_plan, rule, draws):
    """draws uint8 [rows, n], n <= n_plan: the first n draws of the plan -> base positions uint8 [rows, n]"""
    d = np.ascontiguousarray(draws, np.uint8)
    pos = np.full(d.shape, 255, np.uint8)
    rc = lib().hs_epochs_positions(n_plan, rule, d.shape[1], d.ctypes.data_as(C.c_void_p), d.shape[0],
                                   pos.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("hs_epochs_positions: %d (%d draws of %d, rule %d)" % (rc, d.shape[1], n_plan, rule))
    return pos


def rows(queries, seed, first_qid, nopp, ndeal, uniform=False, ways=False, planned=True):
    """Query i (16-byte records) with id first_qid + i through mcq_iteration_sum<.., nopp, ndeal, ..>: -> uint64 [n, 13 or 22]."""
    return hostbuild.rows(lib().hs_epochs_run, queries, 22 if ways else 13, seed, first_qid, nopp, ndeal, int(uniform), int(ways),
                          int(planned), qid_at=1)


def replay_rows(queries, seed32):
    """Parity mode: query i from the start of the MT19937 stream of seed32 -> uint64 [n, 13]."""
    return hostbuild.rows(lib().hs_epochs_replay, queries, 13, seed32)
