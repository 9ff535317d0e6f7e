"""The per-hand entry of the weighted-range-per-seat Monte-Carlo path in the C ABI and the Python surface.  No compute calls
here (no GPU needed)."""
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
    h = header()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", h))
    assert "mcq_eval_batch_ranges_hands" in names and hasattr(L, "mcq_eval_batch_ranges_hands")
    assert any(p[0] == "mcq_eval_batch_ranges_hands" and len(p) == 2 + 11 for p in _lib._PROTOTYPES)
    assert "typedef struct mcq_hand_row" in h and re.search(r"#define MCQ_RANGES_HANDS_MAX_BATCH 1024u", h)
    assert _lib.HAND_ROW_DTYPE.itemsize == 32 and _lib.HAND_ROW_DTYPE.names == ("runs", "win", "tie", "share")
    assert npa.HAND_ROW_DTYPE is _lib.HAND_ROW_DTYPE and _lib.RANGES_HANDS_MAX_BATCH == 1024
    assert "get_range_hand_equities" in mh.__all__ and "get_range_hand_equities" in npa.__all__
    assert callable(npa.get_range_hand_equities) and callable(npa.Engine.eval_batch_ranges_hands)
    # the clause that said the breakdown was missing is gone
    assert "a per-hero-hand breakdown multiway" not in h


def test_refusals_before_a_launch_leave_both_outputs_untouched():
    L = npa.load_library()
    entry = L.mcq_eval_batch_ranges_hands
    board = [4, 17, 22, 30, 41]
    wide = np.ones((1, 1326), np.uint16)
    st = np.zeros((1, 10), np.uint32)
    out = np.full((1, 32), 7, np.uint64)
    hands = np.full((1, 1326, 4), 7, np.uint64)
    good = _lib.pack_query_one([0, 0], board[:3], 3, 10)
    assert entry(None, None, None, None, 0, 0, 1, 0, 0, None, None) == 0          # n == 0: nothing to do
    rc = entry(None, good.ctypes.data, st.ctypes.data, wide.ctypes.data, 1, 1, 1, 0, 0, out.ctypes.data, hands.ctypes.data)
    assert rc == _lib.MCQ_EINVAL and b"mcq_eval_batch_ranges_hands: null context" in L.mcq_last_error()
    # what follows is refused before the context is touched: any non-null pointer will do for it here
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)

    def refused(what, q=good, n=1, seat=0, o=out, h=hands, tables=wide):
        rc = entry(ctx, q.ctypes.data, st.ctypes.data, tables.ctypes.data, len(tables), n, 1, 0, seat,
                   None if o is None else o.ctypes.data, None if h is None else h.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and what in L.mcq_last_error(), (rc, L.mcq_last_error())

    refused(b"null buffer", h=None)
    refused(b"null buffer", o=None)
    refused(b"no seat 3 to watch", seat=3)
    refused(b"no seat 9 to watch", seat=9)
    refused(b"no seat 10 to watch", seat=10)
    refused(b"MCQ_RANGES_HANDS_MAX_BATCH", n=1025)
    # whatever mcq_eval_batch_ranges refuses, under this entry's name
    refused(b"mcq_eval_batch_ranges_hands: record 0 invalid", q=_lib.pack_query_one([0, 0], board[:2], 3, 10))
    none = np.zeros((1, 1326), np.uint16)
    refused(b"no hand of positive weight", tables=none)
    assert (out == 7).all() and (hands == 7).all()


def test_the_wrapper_checks_before_it_calls():
    q = _lib.pack_query_one([0, 0], [4, 17, 22], 3, 100)
    call = npa.Engine.eval_batch_ranges_hands
    tables, seats = np.ones((2, 1326), np.uint16), np.zeros((1, 10), np.uint32)
    for bad in (None, np.ones((2, 1326), np.uint32), np.ones(1326, np.uint16), np.ones((0, 1326), np.uint16)):
        with pytest.raises(ValueError):
            call(None, q, seats, bad, 1)
    for bad in (None, np.zeros((1, 10), np.int32), np.zeros((1, 3), np.uint32), np.zeros((2, 10), np.uint32)):
        with pytest.raises(ValueError):
            call(None, q, bad, tables, 1)
    for seat in (-1, 10):
        with pytest.raises(ValueError):
            call(None, q, seats, tables, 1, seat=seat)
    with pytest.raises(ValueError):
        mh.get_range_hand_equities([0.5, 0.5], ["QC", "7H", "2H"], seat=2)
    with pytest.raises(ValueError):
        mh.get_range_hand_equities([0.5, 0.5], ["2C"] * 6)
