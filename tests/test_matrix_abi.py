"""The hand-against-hand matrix entries in the C ABI and the Python surface.  No compute calls here (no GPU needed): the
records are validated before the context is touched, so every refusal can be checked with outputs full of sentinels."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import matrix_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mcq_exact_matrix", "mcq_exact_matrix_device")


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_entries():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    for entry in ENTRIES:
        assert entry in names and hasattr(L, entry)
    for older in ("mcq_exact_batch_hero_range", "mcq_exact_batch_hero_range_weighted", "mcq_exact_batch_seats"):
        assert older in names and hasattr(L, older)                        # the entries it joins stay
    assert re.search(r"typedef struct mcq_matrix_query \{", header())
    assert re.search(r"#define MCQ_MATRIX_MAX_BATCH 256u", header()) and _lib.MATRIX_MAX_BATCH == 256
    assert len(L.mcq_exact_matrix.argtypes) == 6 and len(L.mcq_exact_matrix_device.argtypes) == 7
    assert list(inspect.signature(npa.Engine.exact_matrix).parameters) == ["self", "queries", "want_tie"]
    assert inspect.signature(npa.Engine.exact_matrix).parameters["want_tie"].default is True
    assert list(inspect.signature(npa.Engine.exact_matrix_device).parameters) == ["self", "queries", "d_win", "d_tie", "stream"]
    assert inspect.signature(npa.Engine.exact_matrix_device).parameters["stream"].default == 0
    for name in ("get_equity_matrix", "matrix_equity"):
        assert name in mh.__all__ and name in npa.__all__ and callable(getattr(npa, name))
    sig = inspect.signature(npa.get_equity_matrix)
    assert list(sig.parameters) == ["table_cards", "dead_cards", "engine"]
    assert sig.parameters["dead_cards"].default == '' and sig.parameters["engine"].default is None
    assert list(inspect.signature(npa.matrix_equity).parameters) == ["win", "tie", "total", "ties"]
    assert inspect.signature(npa.matrix_equity).parameters["ties"].default == "split"
    from neuron_poker_amd import torch_ops
    assert list(inspect.signature(torch_ops.get_equity_matrix_torch).parameters)[:3] == ["boards", "dead", "engine"]


def test_the_record_is_16_bytes_in_c_and_in_numpy(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcq.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(mcq_matrix_query), offsetof(mcq_matrix_query, n_board), offsetof(mcq_matrix_query, reserved), "
                   "offsetof(mcq_matrix_query, dead)); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["16", "5", "6", "8"]
    dt = _lib.MATRIX_QUERY_DTYPE
    assert dt.itemsize == 16 and [dt.fields[k][1] for k in ("board", "n_board", "reserved", "dead")] == [0, 5, 6, 8]
    q = _lib.pack_matrix_query([4, 17, 22], [0, 51])
    assert q["n_board"][0] == 3 and list(q["board"][0]) == [4, 17, 22, 0, 0] and int(q["dead"][0]) == 1 | 1 << 51


def test_the_version_is_still_0_5_0():
    h = header()
    assert [int(re.search(r"#define MCQ_VERSION_%s (\d+)" % k, h).group(1)) for k in ("MAJOR", "MINOR", "PATCH")] == [0, 5, 0]
    L = npa.load_library()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.mcq_version(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (0, 5, 0)


def test_every_refusal_comes_before_the_device_and_writes_nothing():
    L = npa.load_library()
    board, dead = MC.CASES["turn_dead2"][:2]
    good = _lib.pack_matrix_query(board, dead)
    win = np.full(64, 0xA5A5, np.uint16)          # (never written: a refusal must not reach them, and nothing else is tried)
    tie = np.full(64, 0xA5A5, np.uint16)
    total = np.full(4, 0xA5A5A5A5, np.uint32)
    fake = C.create_string_buffer(64)             # refused before the context is touched: any non-null pointer will do
    ctx = C.cast(fake, C.c_void_p)

    def refused(q, n, what, use_win=True, context=ctx):
        for entry in ENTRIES:
            args = [context, None if q is None else q.ctypes.data, n, win.ctypes.data if use_win else None, tie.ctypes.data,
                    total.ctypes.data]
            if entry == "mcq_exact_matrix_device":
                args.append(None)
            assert getattr(L, entry)(*args) == _lib.MCQ_EINVAL, (entry, what)
            assert what in L.mcq_last_error(), (entry, what, L.mcq_last_error())
            assert (win == 0xA5A5).all() and (tie == 0xA5A5).all() and (total == 0xA5A5A5A5).all()

    refused(good, 1, b"null context", context=None)
    refused(good, 0, b"n == 0")
    refused(good, 257, b"MCQ_MATRIX_MAX_BATCH")
    refused(None, 1, b"null records")
    refused(good, 1, b"null win", use_win=False)
    for nb in (0, 1, 2, 6):
        q = good.copy()
        q["n_board"] = nb
        refused(q, 1, b"n_board 3 to 5")
    q = good.copy()
    q["reserved"][0, 1] = 9
    refused(q, 1, b"reserved bytes")
    q = good.copy()
    q["dead"] |= np.uint64(1 << 52)
    refused(q, 1, b"bits 52..63")
    q = good.copy()
    q["board"][0, 0] = 52
    refused(q, 1, b"not below 52")
    q = good.copy()
    q["board"][0, 1] = q["board"][0, 0]
    refused(q, 1, b"given twice")
    refused(_lib.pack_matrix_query(board, dead + [board[0]]), 1, b"also dead")
    refused(_lib.pack_matrix_query(*MC.REFUSED_SHORT), 1, b"L - 4 < k")
    # one bad record refuses the whole batch, and the message names it
    batch = np.concatenate([good, good, _lib.pack_matrix_query(*MC.REFUSED_SHORT)])
    refused(batch, 3, b"record 2:")


def test_python_checks_the_batch_size_before_the_engine():
    class NoEngine:
        _lib = None
        _ctx = None
    for n in (0, 257):
        try:
            npa.Engine.exact_matrix(NoEngine(), np.zeros(n, _lib.MATRIX_QUERY_DTYPE))
        except ValueError as e:
            assert "MATRIX_MAX_BATCH" in str(e)
        else:
            raise AssertionError("n = %d was accepted" % n)


def test_matrix_equity_reads_the_counts():
    win = np.zeros((3, 3), np.uint16)
    tie = np.zeros((3, 3), np.uint16)
    win[0, 1], win[1, 0], tie[0, 1], tie[1, 0] = 6, 2, 2, 2          # total 10; hand 2 meets nobody
    split = mh.matrix_equity(win, tie, 10)
    assert split[0, 1] == 0.7 and split[1, 0] == 0.3 and np.isnan(split[2]).all() and np.isnan(split[0, 0])
    credited = mh.matrix_equity(win, tie, 10, ties="credited")
    assert credited[0, 1] == 0.8 and credited[1, 0] == 0.4
    try:
        mh.matrix_equity(win, tie, 10, ties="half")
    except ValueError:
        pass
    else:
        raise AssertionError("ties='half' was accepted")
