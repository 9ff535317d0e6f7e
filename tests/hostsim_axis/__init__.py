"""Test-only host build of the cost-axis arithmetic of the Monte-Carlo kernels (see hs_axis.cpp)."""
import ctypes as C
import functools

from tests import hostbuild

_U64P, _U32P = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@functools.cache
def lib():
    L = hostbuild.load("hostsim_axis/hs_axis.cpp")
    L.hs_axis_slice.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, _U64P]
    L.hs_axis_slice.restype = None
    L.hs_axis_last_le.argtypes = [_U64P, C.c_uint32, C.c_uint64]
    L.hs_axis_last_le.restype = C.c_uint32
    L.hs_axis_last_lt.argtypes = [_U64P, C.c_uint32, C.c_uint32, C.c_uint64]
    L.hs_axis_last_lt.restype = C.c_uint32
    L.hs_axis_first_task.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.hs_axis_first_task.restype = C.c_uint32
    L.hs_axis_owns.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    L.hs_axis_owns.restype = C.c_int
    L.hs_axis_block_records.argtypes = [_U64P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _U32P]
    L.hs_axis_block_records.restype = None
    L.hs_axis_walk.argtypes = [_U64P, _U32P, _U32P, C.c_uint32, C.c_uint32, C.c_uint32, _U32P, C.c_uint64]
    L.hs_axis_walk.restype = C.c_uint64
    L.hs_axis_partition_exhaustive.argtypes = [C.c_uint32, C.c_uint32, _U32P, C.c_uint32, C.c_uint32, _U64P, _U32P]
    L.hs_axis_partition_exhaustive.restype = C.c_uint64
    return L


def _u64(v):
    return (C.c_uint64 * len(v))(*[int(x) for x in v])


def _u32(v):
    return (C.c_uint32 * len(v))(*[int(x) for x in v])


def slice_of(total, i, n_parts):
    out = (C.c_uint64 * 2)()
    lib().hs_axis_slice(total, i, n_parts, out)
    return int(out[0]), int(out[1])


def last_le(prefix, x):
    return lib().hs_axis_last_le(_u64(prefix), len(prefix) - 1, x)


def last_lt(prefix, start, x):
    return lib().hs_axis_last_lt(_u64(prefix), start, len(prefix) - 1, x)


def first_task(pfx, lo, weight):
    return lib().hs_axis_first_task(pfx, lo, weight)


def owns(pfx, task, weight, hi):
    return bool(lib().hs_axis_owns(pfx, task, weight, hi))


def block_records(prefix, block, waves_per_block, grid):
    """(first record, number of records); the number is 0 for a block without a piece of the axis"""
    out = (C.c_uint32 * 2)()
    lib().hs_axis_block_records(_u64(prefix), len(prefix) - 1, block, waves_per_block, grid, out)
    return int(out[0]), int(out[1])


def walk(tasks, weights, wave, n_waves):
    """the (record, task) pairs wave `wave` of n_waves runs on the axis of records with tasks[i] tasks of weights[i]"""
    prefix = [0]
    for t, w in zip(tasks, weights):
        prefix.append(prefix[-1] + t * w)
    room = sum(tasks) + 1
    out = (C.c_uint32 * (2 * room))()
    k = lib().hs_axis_walk(_u64(prefix), _u32(tasks), _u32(weights), len(tasks), wave, n_waves, out, room)
    assert k <= room
    return [(int(out[2 * j]), int(out[2 * j + 1])) for j in range(k)]


def partition_exhaustive(max_n, max_tasks, weights, max_waves):
    """(cases looked at, cases that are no partition, the first of those)"""
    cases, bad = C.c_uint64(0), (C.c_uint32 * 4)()
    n_bad = lib().hs_axis_partition_exhaustive(max_n, max_tasks, _u32(weights), len(weights), max_waves, C.byref(cases), bad)
    return int(cases.value), int(n_bad), tuple(int(x) for x in bad)
