"""The weighted preflop hero-range entry in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mcq_exact_batch_hero_range_preflop_weighted"


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_entry():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    assert ENTRY in names and hasattr(L, ENTRY)
    for older in ("mcq_exact_batch_hero_range", "mcq_exact_batch_hero_range_preflop", "mcq_exact_batch_hero_range_weighted"):
        assert older in names and hasattr(L, older)                                 # the three entries it joins stay
    assert re.search(r"#define MCQ_COMBO_WEIGHT_MAX 65535u", header()) and _lib.COMBO_WEIGHT_MAX == 65535
    assert re.search(r"#define MCQ_HERO_PREFLOP_MAX_BATCH 64u", header()) and _lib.HERO_PREFLOP_MAX_BATCH == 64
    assert getattr(L, ENTRY).argtypes is not None and len(getattr(L, ENTRY).argtypes) == 8
    assert callable(npa.Engine.exact_hero_range_preflop_weighted)
    assert list(inspect.signature(npa.Engine.exact_hero_range_preflop_weighted).parameters) == [
        "self", "queries", "ext", "opp_weights", "hero_weights"]
    name = "get_preflop_range_equity_exact_weighted"
    assert name in mh.__all__ and name in npa.__all__ and callable(getattr(npa, name))
    sig = inspect.signature(npa.get_preflop_range_equity_exact_weighted)
    assert list(sig.parameters) == ["hero", "opponent", "ghost_cards", "engine", "ties", "by_class"]
    assert sig.parameters["ghost_cards"].default == '' and sig.parameters["engine"].default is None
    assert sig.parameters["ties"].default == "credited" and sig.parameters["by_class"].default is False
    # the postflop weighted entry's comment points here
    assert "Before the flop:\n * mcq_exact_batch_hero_range_preflop_weighted below" in header()


def test_the_version_is_still_0_5_0():
    h = header()
    assert [int(re.search(r"#define MCQ_VERSION_%s (\d+)" % k, h).group(1)) for k in ("MAJOR", "MINOR", "PATCH")] == [0, 5, 0]
    L = npa.load_library()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.mcq_version(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (0, 5, 0)


def test_argument_checks_need_no_device():
    L = npa.load_library()
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.range_bits(["AA"]))
    w = np.ones((1, 1326), np.uint16)
    rows = np.full((1326, 13), 7, np.uint64)
    agg = np.full(11, -1.0)
    entry = getattr(L, ENTRY)
    assert entry(None, None, None, 0, None, None, None, None) == 0                       # n == 0: nothing to do
    assert entry(None, q.ctypes.data, x.ctypes.data, 1, w.ctypes.data, None, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"null context" in L.mcq_last_error()
    # what follows is refused before the context is touched: any non-null pointer will do for it here
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    assert entry(ctx, q.ctypes.data, x.ctypes.data, 1, None, w.ctypes.data, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"null opp_weights" in L.mcq_last_error()
    for args in ((None, x.ctypes.data, rows.ctypes.data), (q.ctypes.data, None, rows.ctypes.data),
                 (q.ctypes.data, x.ctypes.data, None)):
        assert entry(ctx, args[0], args[1], 1, w.ctypes.data, None, args[2], agg.ctypes.data) == _lib.MCQ_EINVAL
        assert b"null buffer" in L.mcq_last_error()
    assert entry(ctx, q.ctypes.data, x.ctypes.data, 65, w.ctypes.data, None, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"MCQ_HERO_PREFLOP_MAX_BATCH" in L.mcq_last_error()
    reasons = []
    flop = _lib.pack_query_one([0, 0], [4, 17, 22], 2, 1)
    reasons.append((flop, x, w, None, b"mcq_exact_batch_hero_range_weighted takes the flop"))
    reasons.append((_lib.pack_query_one([0, 0], [], 3, 1), x, w, None, b"n_players must be 2"))
    reasons.append((_lib.pack_query_one([0, 1], [], 2, 1), _lib.pack_query_ext(1), w, None, b"hero_is_range == 0"))
    xk = x.copy()
    xk["n_known"] = 1
    xk["known"]["cards"][0, 0] = [8, 9]
    reasons.append((_lib.pack_query_one([0, 0], [], 3, 1), xk, w, None, b"n_known must be 0"))
    xe = x.copy()
    xe["opp_range"] = 0
    reasons.append((q, xe, w, None, b"invalid extended query"))
    # no hero hand of positive weight; an opponent without weight; the disjointness refusal: all the opponent's weight on
    # AhAs while the hero may hold AdAh -- decided by the pass over allowed x live pairs, nothing launched
    zeros = np.zeros((1, 1326), np.uint16)
    reasons.append((q, x, w, zeros, b"no hand of the hero's range can be made of the cards left with a positive weight"))
    reasons.append((q, x, zeros, None, b"cannot be dealt against some hand"))
    cid = npa.card_id
    only = zeros.copy()
    only[0, npa.hand_index(cid("AH"), cid("AS"))] = 65535
    reasons.append((q, x, only, None, b"cannot be dealt against some hand"))
    for qq, xx, ow, hw, why in reasons:
        rc = entry(ctx, qq.ctypes.data, xx.ctypes.data, 1, ow.ctypes.data, None if hw is None else hw.ctypes.data, rows.ctypes.data,
                   agg.ctypes.data)
        assert rc == _lib.MCQ_EINVAL, why
        assert why in L.mcq_last_error(), (why, L.mcq_last_error())
    # ... in the second record of a batch likewise
    q2, x2, w2 = np.concatenate([q, q]), np.concatenate([x, x]), np.concatenate([w, only])
    rows2 = np.full((2, 1326, 13), 7, np.uint64)
    assert entry(ctx, q2.ctypes.data, x2.ctypes.data, 2, w2.ctypes.data, None, rows2.ctypes.data, None) == _lib.MCQ_EINVAL
    assert b"query 1:" in L.mcq_last_error() and b"cannot be dealt" in L.mcq_last_error()
    assert (rows == 7).all() and (agg == -1.0).all() and (rows2 == 7).all()


def test_the_wrapper_checks_shape_and_dtype_before_it_calls():
    """Engine.exact_hero_range_preflop_weighted raises ValueError for a wrong table before it touches the engine: no engine
    is needed to see it."""
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES)
    call = npa.Engine.exact_hero_range_preflop_weighted
    good = np.ones((1, 1326), np.uint16)
    for bad in (None, np.ones((1, 1326), np.uint32), np.ones((1, 1326), np.int16), np.ones((1, 1326), np.float64),
                np.ones(1326, np.uint16), np.ones((2, 1326), np.uint16), np.ones((1, 1325), np.uint16), [[1] * 1326]):
        with pytest.raises(ValueError):
            call(None, q, x, bad)
        if bad is not None:
            with pytest.raises(ValueError):
                call(None, q, x, good, bad)
    with pytest.raises(ValueError):
        call(None, q, np.concatenate([x, x]), good)


def test_public_function_refuses_before_it_needs_an_engine():
    f = mh.get_preflop_range_equity_exact_weighted
    with pytest.raises(ValueError):
        f({"AKS"}, 1, ties="half")
    with pytest.raises(ValueError):
        f({"AKS"}, 1, ghost_cards=["AS"])
    with pytest.raises(ValueError):
        f(set(), 1)
    with pytest.raises(ValueError):
        f({"AKS": 0.5}, {"AQX": 1})
    with pytest.raises(ValueError):
        f({"AKS": 0.5}, {"AQO": 1e-7})
