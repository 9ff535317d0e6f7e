"""Test-only host build of the blocks' staging decisions and the candidate lists' compaction steps
(neuron_poker_amd/csrc/mcq_stage.hpp; see hs_stage.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
NOT_WRITTEN = 0xFFFFFFFF
LIST_STRIDE = 2704     # MCQ_EXT_LIST_STRIDE
THREADS = {11: 256, 3: 1024}   # candidates per thread -> threads: mcq_ext_lists_kernel, mcq_eval_ext_small_kernel


@functools.cache
def lib():
    L = hostbuild.load("hostsim_stage/hs_stage.cpp")
    u32, vp = C.c_uint32, C.c_void_p
    L.hs_stage_consts.argtypes = [_U32P]
    L.hs_stage_consts.restype = None
    L.hs_stage_ext_lists.argtypes = [u32, u32, u32, vp, vp]
    L.hs_stage_ranges_slot.argtypes = [_U32P, u32, u32]
    L.hs_stage_ranges_slot.restype = u32
    L.hs_stage_ranges_blocks.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, u32]
    L.hs_stage_ranges_blocks.restype = u32
    L.hs_stage_list_plan.argtypes = [vp, vp, u32, _U64P, vp]
    L.hs_stage_list_plan.restype = None
    L.hs_stage_list_masks.argtypes = [u32, C.c_uint64, vp, vp]
    L.hs_stage_list_masks.restype = u32
    L.hs_stage_list_scatter.argtypes = [u32, vp, vp, vp]
    L.hs_stage_list_scatter.restype = u32
    L.hs_stage_serial_list.argtypes = [vp, vp, u32, vp]
    L.hs_stage_serial_list.restype = u32
    return L


@functools.cache
def consts():
    out = (C.c_uint32 * 4)()
    lib().hs_stage_consts(out)
    return dict(zip(("ext_entries", "ext_lists", "ranges_tables", "ranges_queries"), (int(x) for x in out)))


def ext_lists(first, nq, lists_stride, cnts):
    """mcq_ext_stage_lists -> (staged?, the offsets it wrote: NOT_WRITTEN where it wrote none)"""
    c = np.ascontiguousarray(cnts, np.uint32)
    assert len(c) >= (first + nq) * lists_stride
    off = np.full(consts()["ext_lists"] + 1, NOT_WRITTEN, np.uint32)
    staged = lib().hs_stage_ext_lists(first, nq, lists_stride, c.ctypes.data, off.ctypes.data)
    return bool(staged), [int(x) for x in off]


def ranges_slot(tab_id, t):
    return lib().hs_stage_ranges_slot((C.c_uint32 * len(tab_id))(*tab_id), len(tab_id), t)


def ranges_blocks(queries, seat_table, tables, n_cu, grid_cap=0):
    """The blocks of a ranges batch as the host layer launches it -> (prefix [n + 1], [(first record, records, staged
    table ids), ...] one per block of the grid)."""
    q = np.ascontiguousarray(queries).view(np.uint8).reshape(-1, 16)
    st = np.ascontiguousarray(seat_table, np.uint32)
    t = np.ascontiguousarray(tables, np.uint16)
    assert st.shape == (len(q), 10) and t.ndim == 2 and t.shape[1] == 1326
    prefix = np.zeros(len(q) + 1, np.uint64)
    room = max(n_cu * 2, 1)
    out = np.zeros((room, 9), np.uint32)
    grid = lib().hs_stage_ranges_blocks(q.ctypes.data, st.ctypes.data, t.ctypes.data, len(t), len(q), n_cu, grid_cap,
                                        prefix.ctypes.data, out.ctypes.data, room)
    assert 0 < grid <= room, grid
    blocks = []
    for first, count, n_staged, *ids in out[:grid].tolist():
        assert all(i == NOT_WRITTEN for i in ids[n_staged:]) or n_staged == 0
        blocks.append((first, count, ids[:n_staged]))
    return [int(x) for x in prefix], blocks


def list_plan(query16, ext304, li):
    """(the cards U list li's candidates are made of, its class set as six words)"""
    q, e = hostbuild.record(query16, ext304)
    U, cls = C.c_uint64(0), np.zeros(6, np.uint32)
    lib().hs_stage_list_plan(q.ctypes.data, e.ctypes.data, li, C.byref(U), cls.ctypes.data)
    return int(U.value), cls


def list_masks(per, U, cls):
    """every thread's candidate mask, `per` candidates per thread"""
    cls = np.ascontiguousarray(cls, np.uint32)
    masks = np.zeros(THREADS[per], np.uint32)
    assert len(cls) == 6 and lib().hs_stage_list_masks(per, U, cls.ctypes.data, masks.ctypes.data) == THREADS[per]
    return masks


def list_scatter(per, masks, at, length):
    """the threads' survivors written from their offsets `at` into a list of `length` entries (and a guard entry)"""
    masks, at = np.ascontiguousarray(masks, np.uint32), np.ascontiguousarray(at, np.uint32)
    assert len(masks) == len(at) == THREADS[per]
    dst = np.full(length + 1, 0xFFFF, np.uint16)
    assert lib().hs_stage_list_scatter(per, masks.ctypes.data, at.ctypes.data, dst.ctypes.data) == THREADS[per]
    assert dst[length] == 0xFFFF
    return dst[:length]


def compact(per, U, cls):
    """The two steps with a serial exclusive sum of the threads' counts between them -> the list."""
    masks = list_masks(per, U, cls)
    counts = np.array([bin(int(m)).count("1") for m in masks], np.uint32)
    at = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
    return list_scatter(per, masks, at, int(counts.sum()))


def serial_list(query16, ext304, li):
    """list li of the record as the host builds of the lane code build it (tests/hostsim/hs_walk.hpp)"""
    q, e = hostbuild.record(query16, ext304)
    dst = np.zeros(LIST_STRIDE, np.uint16)
    n = lib().hs_stage_serial_list(q.ctypes.data, e.ctypes.data, li, dst.ctypes.data)
    assert n != NOT_WRITTEN
    return dst[:n]
