"""The hero-range entry in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

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
    assert "mcq_exact_batch_hero_range" in names and hasattr(L, "mcq_exact_batch_hero_range")
    assert re.search(r"#define MCQ_HAND_ROWS 1326u", header()) and _lib.HAND_ROWS == 1326
    assert "get_range_equity_exact" in mh.__all__ and callable(npa.get_range_equity_exact) and callable(npa.hand_index)


def test_hand_index_macro_matches_the_binding(tmp_path):
    """MCQ_HAND_INDEX of the header, compiled as C, against hand_index for all 1326 hands: a bijection onto the rows."""
    src = tmp_path / "hand_index.c"
    src.write_text('#include <stdio.h>\n#include "mcq.h"\nint main(void) {\n    unsigned a, b;\n'
                   '    for (b = 1; b < 52; b++) for (a = 0; a < b; a++) printf("%u\\n", (unsigned)MCQ_HAND_INDEX(a, b));\n'
                   '    printf("%u\\n", (unsigned)MCQ_HAND_ROWS);\n    return 0;\n}\n')
    exe = str(tmp_path / "hand_index")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [npa.hand_index(a, b) for b in range(1, 52) for a in range(b)]
    assert out[:-1] == want and out[-1] == 1326
    assert sorted(want) == list(range(1326))
    assert npa.hand_index(51, 50) == npa.hand_index(50, 51) == 1325 and npa.hand_index(0, 1) == 0
    for bad in ((3, 3), (0, 52), (-1, 4)):
        try:
            npa.hand_index(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_argument_checks_need_no_context():
    L = npa.load_library()
    q = _lib.pack_query_one([0, 0], [4, 17, 22], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.range_bits(["AA"]))
    rows = np.full((1326, 13), 7, np.uint64)
    agg = np.full(11, -1.0)
    entry = L.mcq_exact_batch_hero_range
    assert entry(None, None, None, 0, 0, None, None) == 0                       # n == 0: nothing to do
    assert entry(None, q.ctypes.data, x.ctypes.data, 1, 0, rows.ctypes.data, agg.ctypes.data) == _lib.MCQ_EINVAL
    assert b"null context" in L.mcq_last_error()
    # null buffers are refused before the context is touched: any non-null pointer will do for it here
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    for args in ((None, x.ctypes.data, rows.ctypes.data), (q.ctypes.data, None, rows.ctypes.data),
                 (q.ctypes.data, x.ctypes.data, None)):
        assert entry(ctx, args[0], args[1], 1, 0, args[2], agg.ctypes.data) == _lib.MCQ_EINVAL
        assert b"null buffer" in L.mcq_last_error()
    assert (rows == 7).all() and (agg == -1.0).all()
