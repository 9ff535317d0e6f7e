"""Test-only host build of the preflop hero-range exact enumeration's lane code and its slow reference (see
hs_hero_preflop.cpp)."""
import ctypes as C
import functools

import numpy as np

from tests import hostbuild

ROWS = 1326
SENTINEL = 0xA5A5A5A5A5A5A5A5
REFUSALS = {-2: "empty completion range", -1: "bad law", 1: "invalid", 2: "hero is not a range", 3: "known hands",
            4: "not heads-up", 6: "no allowed hero hand", 7: "range cannot be dealt"}


@functools.cache
def lib():
    L = hostbuild.load("hostsim_hero_preflop/hs_hero_preflop.cpp")
    L.hs_hero_pre.restype = C.c_int
    L.hs_hero_pre_allowed.restype = C.c_int
    L.hs_slow_ref.restype = C.c_int
    L.hs_unrank.restype = None
    L.hs_next.restype = None
    for name in ("hs_binom", "hs_pre_slice", "hs_pre_owned", "hs_pre_max_owned", "hs_pre_share"):
        getattr(L, name).restype = C.c_uint32
    L.hs_pre_slice.argtypes = [C.c_uint64]
    L.hs_pre_owned.argtypes = [C.c_uint32, C.c_uint32]
    L.hs_binom.argtypes = [C.c_uint32, C.c_uint32]
    L.hs_pre_share.argtypes = [C.c_uint32]
    return L


def hero_pre(query16, ext, law=0, lo=0, hi=0xFFFFFFFF):
    """-> (rows[1326, 13] uint64: the partial rows of the completions [lo, hi), agg[11] float64 or None when the range does
    not cover every completion, counts: allowed, live, ranked, completions).  A refusal raises ValueError after checking that
    it left the outputs untouched."""
    q, e = hostbuild.record(query16, ext)
    rows = np.full((ROWS, 13), SENTINEL, np.uint64)
    agg = np.full(11, -7.0, np.float64)
    counts = np.full(4, 0xFFFFFFFF, np.uint32)
    rc = lib().hs_hero_pre(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_int(int(law)), C.c_uint32(lo),
                           C.c_uint32(hi), rows.ctypes.data_as(C.c_void_p), agg.ctypes.data_as(C.c_void_p),
                           counts.ctypes.data_as(C.c_void_p))
    if rc:
        assert (rows == SENTINEL).all() and (agg == -7.0).all() and (counts == 0xFFFFFFFF).all(), "a refusal wrote to the outputs"
        raise ValueError(REFUSALS.get(rc, rc))
    whole = lo == 0 and hi >= int(counts[3])
    assert whole == bool((agg != -7.0).any())
    return rows, (agg if whole else None), [int(v) for v in counts]


def allowed_rows(query16, ext):
    """The rows of the allowed hero hands in the order of the kernel's `allowed` list."""
    q, e = hostbuild.record(query16, ext)
    out = np.zeros(ROWS, np.uint32)
    n = lib().hs_hero_pre_allowed(q.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise ValueError("refused")
    return [int(v) for v in out[:n]]


def unrank(idx, L, k):
    """mcq_exact_unrank of every index -> [n, 5] positions (255 where unused)."""
    idx = np.ascontiguousarray(idx, np.uint32)
    out = np.zeros((len(idx), 5), np.uint32)
    lib().hs_unrank(idx.ctypes.data_as(C.c_void_p), C.c_uint32(len(idx)), C.c_uint32(L), C.c_uint32(k),
                    out.ctypes.data_as(C.c_void_p))
    return out


def step(pos, k):
    """mcq_exact_hero_pre_next of every row of pos[n, 5] -> [n, 5]."""
    pos = np.ascontiguousarray(pos, np.uint32).reshape(-1, 5)
    out = np.zeros_like(pos)
    lib().hs_next(pos.ctypes.data_as(C.c_void_p), C.c_uint32(len(pos)), C.c_uint32(k), out.ctypes.data_as(C.c_void_p))
    return out


def slow_ref(deck, opp_bits, law, start, count, hands):
    """The slow reference: deck = D's card ids ascending, opp_bits = the opponent's 6-word range, start = the D-positions
    (ascending) of the first completion, count = how many completions follow in index order, hands = [(a, b)] card ids.
    -> rows[len(hands), 13] uint64."""
    d = np.ascontiguousarray(deck, np.uint8)
    bits = np.ascontiguousarray(opp_bits, np.uint32)
    st = np.ascontiguousarray(start, np.uint32)
    h = np.ascontiguousarray(hands, np.uint8).reshape(-1, 2)
    assert len(st) == 5 and len(bits) == 6 and (h[:, 0] < h[:, 1]).all()
    rows = np.zeros((len(h), 13), np.uint64)
    rc = lib().hs_slow_ref(d.ctypes.data_as(C.c_void_p), C.c_uint32(len(d)), bits.ctypes.data_as(C.c_void_p), C.c_int(int(law)),
                           st.ctypes.data_as(C.c_void_p), C.c_uint32(count), h.ctypes.data_as(C.c_void_p), C.c_uint32(len(h)),
                           rows.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return rows
