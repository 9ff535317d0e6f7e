"""The preflop hero-range entry in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mcq_exact_batch_hero_range_preflop"


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_entry():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    assert ENTRY in names and hasattr(L, ENTRY)
    assert "mcq_exact_batch_hero_range" in names                                   # the postflop entry stays
    assert re.search(r"#define MCQ_HERO_PREFLOP_MAX_BATCH 64u", header()) and _lib.HERO_PREFLOP_MAX_BATCH == 64
    assert callable(getattr(npa.Engine, "exact_hero_range_preflop"))
    for name in ("get_preflop_range_equity_exact", "preflop_class_table"):
        assert name in mh.__all__ and name in npa.__all__ and callable(getattr(npa, name))
    sig = inspect.signature(npa.get_preflop_range_equity_exact)
    assert list(sig.parameters) == ["hero_range", "opponent_range", "dealing", "ghost_cards", "engine", "ties", "by_class"]
    assert sig.parameters["opponent_range"].default == 1 and sig.parameters["by_class"].default is False


def test_the_lane_code_is_a_header_of_its_own_and_the_others_are_included():
    with open(os.path.join(ROOT, "neuron_poker_amd", "csrc", "mcq_exact_hero_pre.hpp")) as f:
        text = f.read()
    assert '#include "mcq_exact_hero.hpp"' in text and "static_assert" in text
    with open(os.path.join(ROOT, "neuron_poker_amd", "csrc", "Makefile")) as f:
        assert "mcq_exact_hero_pre.hpp" in f.read()                                # a change of it rebuilds the library


def test_argument_checks_need_no_context():
    L = npa.load_library()
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.range_bits(["AA"]))
    rows = np.full((1326, 13), 7, np.uint64)
    agg = np.full(11, -1.0)
    entry = getattr(L, ENTRY)
    assert entry(None, None, None, 0, 0, None, None) == 0                       # n == 0: nothing to do
    assert entry(None, q.ctypes.data, x.ctypes.data, 1, 0, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"null context" in L.mcq_last_error()
    # null buffers, a bad law, too many records and a record that cannot be enumerated are refused before the context is
    # touched: any non-null pointer will do for it here
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    for args in ((None, x.ctypes.data, rows.ctypes.data), (q.ctypes.data, None, rows.ctypes.data),
                 (q.ctypes.data, x.ctypes.data, None)):
        assert entry(ctx, args[0], args[1], 1, 0, args[2], agg.ctypes.data) == _lib.MCQ_EINVAL
        assert b"null buffer" in L.mcq_last_error()
    assert entry(ctx, q.ctypes.data, x.ctypes.data, 1, 2, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"bad law" in L.mcq_last_error()
    assert entry(ctx, q.ctypes.data, x.ctypes.data, 65, 0, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"MCQ_HERO_PREFLOP_MAX_BATCH" in L.mcq_last_error()
    reasons = []
    flop = _lib.pack_query_one([0, 0], [4, 17, 22], 2, 1)
    reasons.append((flop, x, b"mcq_exact_batch_hero_range takes the flop"))
    reasons.append((_lib.pack_query_one([0, 0], [], 3, 1), x, b"n_players must be 2"))
    reasons.append((_lib.pack_query_one([0, 1], [], 2, 1), _lib.pack_query_ext(1), b"hero_is_range == 0"))
    xk = x.copy()
    xk["n_known"] = 1
    xk["known"]["cards"][0, 0] = [8, 9]
    reasons.append((_lib.pack_query_one([0, 0], [], 3, 1), xk, b"n_known must be 0"))
    xe = x.copy()
    xe["opp_range"] = 0
    reasons.append((q, xe, b"invalid extended query"))
    for qq, xx, why in reasons:
        assert entry(ctx, qq.ctypes.data, xx.ctypes.data, 1, 0, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL, why
        assert why in L.mcq_last_error(), (why, L.mcq_last_error())
    assert (rows == 7).all() and (agg == -1.0).all()
