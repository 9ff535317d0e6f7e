"""Test-only host build of the launch plans (neuron_poker_amd/csrc/mcq_plan.hpp; see hs_plan.cpp) and the fixture rows
of plan_rows.inc."""
import ctypes as C
import functools
import os
import re

import numpy as np

from tests import hostbuild

_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_HERE = os.path.dirname(os.path.abspath(__file__))
ROW_KINDS = ("PLAN_GEOMETRY", "PLAN_SMALL_CUT", "PLAN_EXACT", "PLAN_EXACT_EXT", "PLAN_PRICE")   # hs_plan_row's numbers


@functools.cache
def lib():
    L = hostbuild.load("hostsim_plan/hs_plan.cpp")
    u32 = C.c_uint32
    L.hs_plan_geometry.argtypes = [u32] * 5 + [C.c_int, C.c_uint64, C.c_uint64, _U32P]
    L.hs_plan_pick_split.argtypes = [C.c_uint64, C.c_uint64, u32, u32]
    L.hs_plan_pick_split.restype = u32
    L.hs_plan_small_cut.argtypes = [C.c_uint64, u32, u32, _U32P]
    L.hs_plan_ext_small_limits.argtypes = [_U32P]
    L.hs_plan_ext_small_fits.argtypes = [C.c_uint64, u32, u32]
    L.hs_plan_ext_small_fits.restype = C.c_int
    L.hs_plan_ext_small.argtypes = [_U32P, u32, _U32P, _U32P, _U32P]
    L.hs_plan_ext_small.restype = u32
    L.hs_plan_with_card.argtypes = [C.c_void_p, _U32P]
    L.hs_plan_ranges_price.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, _U32P, _U32P]
    L.hs_plan_table.argtypes = [u32] * 4 + [C.c_void_p]
    L.hs_plan_exact.argtypes = [C.c_char_p, u32, u32, _U32P]
    L.hs_plan_exact_ext.argtypes = [C.c_char_p] + [u32] * 6 + [_U32P]
    L.hs_plan_exact_hero.argtypes = [C.c_int, C.c_char_p] + [u32] * 6 + [_U32P]
    L.hs_plan_row.argtypes = [u32, _U64P, C.c_uint64]
    L.hs_plan_row.restype = C.c_int
    for f in (L.hs_plan_geometry, L.hs_plan_small_cut, L.hs_plan_ext_small_limits, L.hs_plan_with_card, L.hs_plan_ranges_price,
              L.hs_plan_table, L.hs_plan_exact, L.hs_plan_exact_ext, L.hs_plan_exact_hero):
        f.restype = None
    return L


def _out(fn, n, *args):
    out = (C.c_uint32 * n)()
    fn(*args, out)
    return tuple(int(x) for x in out)


def _q16(q):
    return hostbuild.first_bytes(q, 16).tobytes()


def geometry(total_tasks, n_cu, occ, bulk=False, max_tasks=0, grid_cap=0, split_max=4, load_waves=16):
    """mcq_plan_geometry -> (grid, block, split, work_wpb)"""
    return _out(lib().hs_plan_geometry, 4, n_cu, occ, grid_cap, split_max, load_waves, int(bulk), total_tasks, max_tasks)


def pick_split(total_tasks, max_tasks, n_cu, split_max):
    return lib().hs_plan_pick_split(total_tasks, max_tasks, n_cu, split_max)


def small_cut(n, n_cu, split_max=4):
    """mcq_plan_small_cut -> (lg, grid, rounds)"""
    return _out(lib().hs_plan_small_cut, 3, n, n_cu, split_max)


def ext_small_limits():
    """MCQ_EXT_SMALL_Q, _LISTS, _TASKS, _BLOCKS"""
    return _out(lib().hs_plan_ext_small_limits, 4)


def ext_small_fits(n, lists_stride, most_tasks):
    return bool(lib().hs_plan_ext_small_fits(n, lists_stride, most_tasks))


def ext_small_plan(tasks):
    """mcq_ext_small_plan of a batch that fits -> (wpb, [(query, part, parts, wpb) per block], first_block [n + 1])"""
    n = len(tasks)
    blk, first, n_blocks = (C.c_uint32 * 128)(), (C.c_uint32 * (n + 1))(), C.c_uint32(0)
    wpb = lib().hs_plan_ext_small((C.c_uint32 * n)(*tasks), n, blk, first, C.byref(n_blocks))
    assert wpb, "a block word does not survive unpacking and packing"
    return wpb, [tuple(int(x) for x in blk[4 * b:4 * b + 4]) for b in range(n_blocks.value)], [int(x) for x in first]


def with_card(table):
    t = np.ascontiguousarray(table, np.uint16)
    assert t.shape == (1326,)
    return np.array(_out(lib().hs_plan_with_card, 53, t.ctypes.data), np.int64)


def ranges_price(tables, q, seat_row):
    """mcq_ranges_price of one record -> (price, refused, seat, table)"""
    t = np.ascontiguousarray(tables, np.uint16)
    assert t.ndim == 2 and t.shape[1] == 1326 and len(seat_row) <= 10
    seats = (C.c_uint32 * 10)(*seat_row)
    return _out(lib().hs_plan_ranges_price, 4, t.ctypes.data, len(t), _q16(q), seats)


def synthetic_table(kind, a, b, w):
    """The table (kind, a, b, w) of a price row as hs_rows.hpp builds it."""
    t = np.zeros(1326, np.uint16)
    lib().hs_plan_table(kind, a, b, w, t.ctypes.data)
    return t


def exact_plan(q, n_cu, row=0):
    """mcq_exact_plan -> (n_boards, slices, row, grid)"""
    out = _out(lib().hs_plan_exact, 4, _q16(q), row, n_cu)
    assert out[3] != 0xFFFFFFFF, "the job does not carry the record"
    return out


def exact_ext_plan(q, kind, L, n_cu, ext=0, row=0, h1_off=0):
    """mcq_exact_ext_plan -> (returned grid, ext, n_boards, row, grid, groups, h1_off)"""
    return _out(lib().hs_plan_exact_ext, 7, _q16(q), ext, row, kind, L, h1_off, n_cu)


def exact_hero_plan(preflop, q, L, n_allowed, n_cu, slice_=0, ext=0, row=0):
    """mcq_exact_hero_plan -> (returned grid or 0, ext, n_boards, row, grid, groups, h1_off)"""
    return _out(lib().hs_plan_exact_hero, 7, int(preflop), _q16(q), ext, row, L, n_allowed, n_cu, slice_)


@functools.cache
def rows():
    """plan_rows.inc -> {row kind: [tuple of integers, ...]}"""
    out = {k: [] for k in ROW_KINDS}
    with open(os.path.join(_HERE, "plan_rows.inc")) as f:
        for line in f:
            m = re.match(r"(PLAN_[A-Z_]+)\(([0-9, ]+)\)", line)
            if m:
                out[m.group(1)].append(tuple(int(x) for x in m.group(2).split(",")))
            else:
                assert line.startswith(("//", "/*")), line
    return out


def row_holds(kind, row):
    """Does the header give the row's results (its first columns) for its inputs (the rest)?"""
    return bool(lib().hs_plan_row(ROW_KINDS.index(kind), (C.c_uint64 * len(row))(*row), len(row)))
