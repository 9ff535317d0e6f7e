"""The weighted-range-per-seat Monte-Carlo entry in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
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
    assert "mcq_eval_batch_ranges" in names and hasattr(L, "mcq_eval_batch_ranges")
    assert "get_range_equities" in mh.__all__ and "get_range_equities" in npa.__all__ and callable(npa.get_range_equities)
    assert callable(npa.Engine.eval_batch_ranges)
    h = header()
    assert "JOINT law" in h and "WHOLE trial is abandoned" in h and "Ten wide ranges are expensive" in h


def test_the_version_is_still_0_5_0():
    h = header()
    assert [int(re.search(r"#define MCQ_VERSION_%s (\d+)" % k, h).group(1)) for k in ("MAJOR", "MINOR", "PATCH")] == [0, 5, 0]
    L = npa.load_library()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.mcq_version(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (0, 5, 0)


def test_refusals_before_a_launch_leave_out_untouched():
    L = npa.load_library()
    entry = L.mcq_eval_batch_ranges
    board = [4, 17, 22, 30, 41]
    wide = np.ones((2, 1326), np.uint16)
    wide[1] = 0
    wide[1, _lib.hand_index(4, 50)] = 9          # table 1: one hand, and it holds table card 4
    st = np.zeros((1, 10), np.uint32)
    st[0, 2:] = 1000                             # entries at or above n_players are ignored
    out = np.full((1, 32), 7, np.uint64)
    good = _lib.pack_query_one([0, 0], board[:3], 2, 10)
    assert entry(None, None, None, None, 0, 0, 1, 0, None) == 0          # n == 0: nothing to do
    assert entry(None, good.ctypes.data, st.ctypes.data, wide.ctypes.data, 2, 1, 1, 0, out.ctypes.data) == _lib.MCQ_EINVAL
    assert b"null context" in L.mcq_last_error()
    # what follows is refused before the context is touched: any non-null pointer will do for it here
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)

    def refused(q, seats=st, tables=wide, n_tables=2, o=out, what=b"mcq_eval_batch_ranges"):
        rc = entry(ctx, None if q is None else q.ctypes.data, None if seats is None else seats.ctypes.data,
                   None if tables is None else tables.ctypes.data, n_tables, 1, 1, 0, None if o is None else o.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and what in L.mcq_last_error(), (rc, L.mcq_last_error())

    for args in (dict(q=None), dict(q=good, seats=None), dict(q=good, tables=None), dict(q=good, o=None)):
        refused(what=b"null buffer", **args)
    refused(good, n_tables=0, what=b"n_tables")
    bad_records = [
        _lib.pack_query_one([0, 0], [4, 4, 22], 2, 10),          # a duplicate table card
        _lib.pack_query_one([0, 0], [4, 52, 22], 2, 10),         # a table card out of range
        _lib.pack_query_one([0, 0], board[:1], 2, 10),           # n_board 1
        _lib.pack_query_one([0, 0], board[:2], 2, 10),           # n_board 2
        _lib.pack_query_one([0, 0], board[:3], 1, 10),           # n_players outside 2..10
        _lib.pack_query_one([0, 0], board[:3], 11, 10),
        _lib.pack_query_one([0, 0], board[:3], 2, 0),            # runs == 0
    ]
    r = good.copy()
    r["reserved"][0, 1] = 1
    bad_records.append(r)                                        # non-zero reserved
    for q in bad_records:
        refused(q, what=b"invalid")
    refused(_lib.pack_query_one([3, 3], board, 2, 10).copy(), seats=np.full((1, 10), 2, np.uint32), what=b"names table 2 of 2")
    st1 = st.copy()
    st1[0, 1] = 1
    refused(good, seats=st1, what=b"no hand of positive weight clear of the table cards")
    assert (out == 7).all()
    # hole is ignored: a record whose hole cards are on the table is a valid record (refused here only for its table 1)
    refused(_lib.pack_query_one([4, 4], board[:3], 2, 10), seats=st1, what=b"seat 1")


def test_the_wrapper_checks_shape_and_dtype_before_it_calls():
    q = _lib.pack_query_one([0, 0], [4, 17, 22], 3, 100)
    call = npa.Engine.eval_batch_ranges
    tables, seats = np.ones((2, 1326), np.uint16), np.zeros((1, 10), np.uint32)
    for bad in (None, np.ones((2, 1326), np.uint32), np.ones((2, 1326), np.int16), np.ones((2, 1326), np.float64),
                np.ones(1326, np.uint16), np.ones((2, 1325), np.uint16), np.ones((0, 1326), np.uint16), [[1] * 1326]):
        with pytest.raises(ValueError):
            call(None, q, seats, bad, 1)
    for bad in (None, np.zeros((1, 10), np.int32), np.zeros((1, 10), np.uint64), np.zeros((1, 3), np.uint32),
                np.zeros(10, np.uint32), np.zeros((2, 10), np.uint32), [[0] * 10]):
        with pytest.raises(ValueError):
            call(None, q, bad, tables, 1)


def test_get_range_equities_builds_shared_tables():
    cid = npa.card_id
    top = 0.25
    tables, seat_table = mh._range_tables([("AH", "KH"), top, {"AKS", "QQ"}, top, {"QQ": 1.0, "AKS": 1.0}, ("KH", "AH")])
    assert tables.dtype == np.uint16 and tables.shape == (4, 1326) and seat_table.dtype == np.uint32 and seat_table.shape == (1, 10)
    assert list(seat_table[0]) == [0, 1, 2, 1, 3, 0, 0, 0, 0, 0]
    assert int(tables[0].sum()) == 65535 and tables[0, npa.hand_index(cid("AH"), cid("KH"))] == 65535
    # a plain range is the 0/1 table of its class bits; the same classes as a dict weigh COMBO_WEIGHT_MAX
    assert set(np.unique(tables[1])) == {0, 1} and int(tables[2].sum()) == 4 + 6 and int((tables[3] == 65535).sum()) == 10
    assert np.array_equal(tables[2] != 0, tables[3] != 0)
    bits = mh._opponent_range_bits(top)
    hands = [(a, b) for b in range(52) for a in range(b)]
    for i in (0, 5, 700, 1325):
        bit = _lib.class_bit(mh._hand_class(*hands[i]))
        assert int(tables[1, i]) == (int(bits[bit >> 5]) >> (bit & 31)) & 1
    assert int(tables[1].sum()) == sum(12 if c[0] != c[1] and c[2:] == "O" else 4 if c[0] != c[1] else 6
                                       for c in mh._class_order()[-int(169 * top):])
    for bad in ([("AH", "KH")], [0.5] * 11, [("AH", "AH"), 0.5], [{"AQX": 1.0}, 0.5]):
        with pytest.raises(ValueError):
            mh._range_tables(bad)
    with pytest.raises(ValueError):
        mh.get_range_equities([0.5, 0.5], ["2C"] * 6)
