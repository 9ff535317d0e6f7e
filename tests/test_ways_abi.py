"""The split-pot entries in the C ABI and the Python surface.  No compute calls here (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_ways_entries():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    for n in ("mcq_eval_batch_ways", "mcq_eval_batch_device_ways"):
        assert n in names and hasattr(L, n), n


def test_version_is_0_5_0_in_header_and_library():
    L = npa.load_library()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.mcq_version(C.byref(a), C.byref(b), C.byref(c))
    h = header()
    hv = tuple(int(re.search(r"#define MCQ_VERSION_%s (\d+)" % k, h).group(1)) for k in ("MAJOR", "MINOR", "PATCH"))
    assert hv == (0, 5, 0) and (a.value, b.value, c.value) == (0, 5, 0)


def test_ways_row_layout_matches_the_header(tmp_path):
    from neuron_poker_amd import build
    build.build()
    d = _lib.RESULT_WAYS_DTYPE
    assert d.itemsize == 176 and d.fields["tie_ways"][1] == 104 and d.fields["tie_ways"][0].shape == (9,)
    for name in _lib.RESULT_DTYPE.names:     # the first 104 bytes are an mcq_result
        assert d.fields[name][1] == _lib.RESULT_DTYPE.fields[name][1]
    exe = str(tmp_path / "equity")
    lib = npa.library_path()
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "equity.c"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert [int(x) for x in subprocess.check_output([exe, "--layout-ways"]).split()] == [176]


def test_bad_ties_argument_raises_before_touching_the_gpu():
    hole, board = np.array([[50, 46]], np.uint8), np.full((1, 5), 255, np.uint8)
    with pytest.raises(ValueError):
        mh.get_equity_batch(hole, board, 2, 100, seed=1, ties="bogus")
    with pytest.raises(ValueError):
        mh.get_equity_batch(hole, board, 2, 100, seed=1, ties="split", devices=[0, 0])
    assert "get_pot_equity" in mh.__all__ and callable(mh.get_pot_equity)
