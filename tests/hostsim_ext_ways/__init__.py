"""Test-only host build of the extended lane code with the split-pot switch on (see hs_ext_ways.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild


@functools.cache
def lib():
    L = hostbuild.load("hostsim_ext_ways/hs_ext_ways.cpp")
    L.hs_ext_ways_run.restype = C.c_int
    L.hs_ext_ways_is_fast.restype = C.c_int
    L.hs_exact_ext_ways.restype = C.c_int
    return L


def run(replay, query16, ext304, seed, qid=0, general=False, hands=False):
    """One extended query through the lane code -> the 22 words of its mcq_result_ways row (and, with hands=True, every
    iteration's dealt hands: [runs, 2 * n_players + 5] card ids, the five table cards last).  replay: the caller passes
    seed = (seed + qid) mod 2^32, as the library's parity mode seeds a query."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(22, np.uint64)
    runs, n_players = int(q[12:16].view("<u4")[0]), int(q[8])
    tr = np.full((max(runs, 1), 2 * n_players + 5), 255, np.uint8) if hands else None
    rc = lib().hs_ext_ways_run(C.c_int(1 if replay else 0), q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                               C.c_uint64(seed), C.c_uint64(qid), C.c_int(1 if general else 0),
                               out.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p) if hands else None)
    if rc:
        raise ValueError(rc)
    return (out, tr[:runs]) if hands else out


def is_fast(query16, ext304):
    q, e = hostbuild.record(query16, ext304)
    return bool(lib().hs_ext_ways_is_fast(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p)))


def _u32(name, query16, ext304, *more):
    q, e = hostbuild.record(query16, ext304)
    f = getattr(lib(), name)
    f.restype = C.c_uint32
    return int(f(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), *[C.c_uint32(m) for m in more]))


def n_lists(query16, ext304):
    """mcq_ext_n_lists: the candidate lists the query draws from."""
    return _u32("hs_ext_n_lists", query16, ext304)


def stream_iters(query16, ext304):
    """mcq_ext_stream_iters: 2 or 16 iterations per stream (MCQ-CTR v5x)."""
    return _u32("hs_ext_stream_iters", query16, ext304)


def task_count(query16, ext304):
    """mcq_ext_task_count under the query's stream rule: its wave tasks."""
    return _u32("hs_ext_task_count", query16, ext304)


def task_weight(query16, ext304):
    """mcq_ext_task_weight under the query's stream rule: what one wave task costs on the kernels' cost axis."""
    return _u32("hs_ext_task_weight", query16, ext304)


def list_len(query16, ext304, li):
    """Entries of candidate list li as mcq_ext_lists_kernel lays it out (0: the query has no such list)."""
    return _u32("hs_ext_list_len", query16, ext304, li)


def exact(query16, ext304, law):
    """The exact split-pot lane code (kinds 0 and 1) -> 22 words of integer weights; ValueError(code) on a refusal."""
    q, e = hostbuild.record(query16, ext304)
    out = np.zeros(22, np.uint64)
    rc = lib().hs_exact_ext_ways(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(law),
                                 out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(rc)
    return out
