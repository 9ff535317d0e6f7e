"""The per-seat record and its two entries in the C ABI and the Python binding.  No compute calls here (no GPU needed)."""
import os
import re
import subprocess

import neuron_poker_amd as npa
from neuron_poker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mcq_eval_batch_ext_seats", "mcq_exact_batch_seats")


def header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_seats_row_layout_in_the_binding():
    d = _lib.RESULT_SEATS_DTYPE
    assert npa.RESULT_SEATS is d and d.itemsize == 256
    assert d.fields["runs"][1] == 0 and d.fields["passes"][1] == 8 and d.fields["seat"][1] == 16
    seat = d.fields["seat"][0]
    assert seat.shape == (10,) and seat.base.itemsize == 24
    assert [seat.base.fields[n][1] for n in ("win", "tie", "share")] == [0, 8, 16]
    assert _lib.SHARE_UNIT == 2520 and all(2520 % k == 0 for k in range(1, 11))


def test_header_is_plain_c_with_the_same_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mcq.h"\n'
                   '_Static_assert(sizeof(mcq_result_seats) == 256, "size");\n'
                   '_Static_assert(sizeof(mcq_seat) == 24, "seat");\n'
                   '_Static_assert(offsetof(mcq_result_seats, runs) == 0 && offsetof(mcq_result_seats, passes) == 8, "head");\n'
                   '_Static_assert(offsetof(mcq_result_seats, seat) == 16, "seats");\n'
                   '_Static_assert(offsetof(mcq_seat, win) == 0 && offsetof(mcq_seat, tie) == 8 && offsetof(mcq_seat, share) == 16, "seat fields");\n'
                   '_Static_assert(MCQ_SHARE_UNIT == 2520u, "unit");\n'
                   'int main(void) { return 0; }\n')
    # (_Static_assert is C11; the header itself is held to C99 by the second compile)
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "layout.o")])
    only = tmp_path / "only.c"
    only.write_text('#include "mcq.h"\nint main(void) { return (int)sizeof(mcq_result_seats) - 256; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(only), "-o", str(tmp_path / "only.o")])


def test_entries_declared_and_exported():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    names = set(re.findall(r"MCQ_API\s+[\w\s\*]+?\b(mcq_\w+)\s*\(", header()))
    for n in ENTRIES:
        assert n in names and hasattr(L, n), n
    h = header()
    assert "MCQ_MODE_PHILOX only" in h and "random opponent" in h   # the two limits are stated where the entries are declared


def test_c_example_reports_the_row_size(tmp_path):
    from neuron_poker_amd import build
    build.build()
    exe = str(tmp_path / "equity")
    lib = npa.library_path()
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "equity.c"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert [int(x) for x in subprocess.check_output([exe, "--layout-seats"]).split()] == [_lib.RESULT_SEATS_DTYPE.itemsize] == [256]


def test_python_surface_without_gpu():
    import numpy as np
    import pytest
    from neuron_poker_amd import montecarlo_hip as mh
    assert callable(npa.get_seat_equities) and npa.get_seat_equities is mh.get_seat_equities and "get_seat_equities" in mh.__all__
    rows = np.zeros((2, 32), np.uint64)
    rows[0, 0], rows[0, 4], rows[0, 7] = 10, 2520 * 4, 2520 * 6
    rows[1, 0], rows[1, 4], rows[1, 7], rows[1, 10] = 3, 2520 + 840, 2520 + 840, 840
    s = npa.seat_shares(rows)
    assert s.shape == (2, 10) and list(s[0, :3]) == [0.4, 0.6, 0.0] and s[1, :3].sum() == pytest.approx(1.0, abs=1e-15)
    n = npa.seat_shares(rows.view(npa.RESULT_SEATS).reshape(2), n_players=[2, 3])
    assert np.isnan(n[0, 2:]).all() and np.isnan(n[1, 3:]).all() and not np.isnan(n[1, :3]).any()
    with pytest.raises(ValueError):   # exact=True enumerates known hands only: raised before anything touches the GPU
        mh.get_seat_equities([["AH", "KD"], ["QS", "QC"]], [], 3, exact=True)
