"""The weighted hero-range entry in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_entry():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    assert "mcq_exact_batch_hero_range_weighted" in names and hasattr(L, "mcq_exact_batch_hero_range_weighted")
    assert re.search(r"#define MCQ_COMBO_WEIGHT_MAX 65535u", header()) and _lib.COMBO_WEIGHT_MAX == 65535
    for name in ("get_range_equity_exact_weighted",):
        assert name in mh.__all__ and name in npa.__all__ and callable(getattr(npa, name))
    assert callable(npa.Engine.exact_hero_range_weighted)


def test_the_version_is_still_0_5_0():
    h = header()
    assert [int(re.search(r"#define MCQ_VERSION_%s (\d+)" % k, h).group(1)) for k in ("MAJOR", "MINOR", "PATCH")] == [0, 5, 0]
    L = npa.load_library()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.mcq_version(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (0, 5, 0)


def test_argument_checks_need_no_device():
    L = npa.load_library()
    q = _lib.pack_query_one([0, 0], [4, 17, 22], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.range_bits(["AA"]))
    w = np.ones((1, 1326), np.uint16)
    rows = np.full((1326, 13), 7, np.uint64)
    agg = np.full(11, -1.0)
    entry = L.mcq_exact_batch_hero_range_weighted
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
    assert entry(ctx, q.ctypes.data, x.ctypes.data, 1025, w.ctypes.data, None, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"MCQ_HERO_RANGE_MAX_BATCH" in L.mcq_last_error()
    assert re.search(r"#define MCQ_HERO_RANGE_MAX_BATCH 1024u", header())
    assert (rows == 7).all() and (agg == -1.0).all()


def test_the_wrapper_checks_shape_and_dtype_before_it_calls():
    """Engine.exact_hero_range_weighted raises ValueError for a wrong table before it touches the engine: no engine is
    needed to see it."""
    q = _lib.pack_query_one([0, 0], [4, 17, 22], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES)
    call = npa.Engine.exact_hero_range_weighted
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


def test_weight_quantisation():
    Q = mh.quantise_weight
    assert [Q(0), Q(1), Q(0.5), Q(0.25), Q(0.12)] == [0, 65535, 32768, 16384, 7864]
    assert Q(1 / 65535.0) == 1 and Q(0.6 / 65535.0) == 1 and Q(1.4 / 65535.0) == 1 and Q(1.6 / 65535.0) == 2
    for bad in (0.4 / 65535.0, 1e-9, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            Q(bad)
    # a dict: a class entry for all its hands, a hand entry overrides it, whatever is not named weighs 0
    bits, table = mh._weighted_range({"AQO": 0.5, "QAS": 1, ("AH", "QS"): 0.25, ("KH", "KS"): 1.0}, "opponent")
    assert (np.asarray(bits) == _lib.ALL_CLASSES).all() and table.shape == (1, 1326) and table.dtype == np.uint16
    cid = npa.card_id
    assert table[0, npa.hand_index(cid("AH"), cid("QS"))] == 16384
    assert table[0, npa.hand_index(cid("AS"), cid("QH"))] == 32768
    assert table[0, npa.hand_index(cid("AS"), cid("QS"))] == 65535
    assert table[0, npa.hand_index(cid("KH"), cid("KS"))] == 65535 and table[0, npa.hand_index(cid("KH"), cid("KD"))] == 0
    assert int((table != 0).sum()) == 12 + 4 + 1
    for bad in ({"AQX": 1}, {("AH",): 1}, {"AQO": 2}, {"AQO": 1e-7}):
        with pytest.raises(ValueError):
            mh._weighted_range(bad, "hero")
    # a plain range: its classes, every hand 1
    bits, table = mh._weighted_range({"AKS", "QQ"}, "hero")
    assert table is None and (np.asarray(bits) == _lib.range_bits(["AKS", "QQ"])).all()
    bits, table = mh._weighted_range(1, "hero")
    assert table is None and (np.asarray(bits) == _lib.ALL_CLASSES).all()
