"""The ctypes binding (neuron_poker_amd/_lib.py) against include/mcq.h: every prototype of its table is the header's,
argument errors are raised before the engine is touched, return codes map to the documented exceptions.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declarations():
    """-> [(name, return type, [parameter, ...])] of every MCQ_API function of include/mcq.h, comments stripped."""
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for ret, name, params in re.findall(r"\bMCQ_API\s+([\w\s\*]+?)\b(mcq_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out.append((name, " ".join(ret.split()), [] if params == "void" else [p.strip() for p in params.split(",")]))
    return out


SCALARS = {"size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}


def parameter_type(decl):
    """A C parameter declaration -> "pointer" or the ctypes scalar; anything else fails the test."""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == 2 and words[0] in SCALARS, "include/mcq.h: no ctypes type known for parameter %r" % decl
    return SCALARS[words[0]]


def return_type(decl):
    decl = " ".join(decl.replace("*", " * ").split())
    if decl == "const char *":
        return C.c_char_p
    if decl.endswith("*"):
        return C.c_void_p
    known = {"void": None, "float": C.c_float, **SCALARS}
    assert decl in known, "include/mcq.h: no ctypes type known for return type %r" % decl
    return known[decl]


def is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_every_prototype_is_the_headers():
    from neuron_poker_amd import build
    build.build()
    L = npa.load_library()
    decls = declarations()
    assert len(decls) >= 48
    names = [d[0] for d in decls]
    assert len(set(names)) == len(names)
    table = [p[0] for p in _lib._PROTOTYPES]
    assert table == names                       # the header's functions, no more and no fewer, in the header's order
    for name, ret, params in decls:
        fn = getattr(L, name)
        assert fn.restype == return_type(ret), (name, ret, fn.restype)
        assert len(fn.argtypes) == len(params), (name, params, fn.argtypes)
        for have, decl in zip(fn.argtypes, params):
            want = parameter_type(decl)
            assert is_pointer(have) if want == "pointer" else have is want, (name, decl, have)


def test_a_symbol_the_library_lacks_fails_the_load_by_name(monkeypatch):
    assert os.path.exists(npa.library_path())
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_PROTOTYPES", _lib._PROTOTYPES + (("mcq_no_such_entry", C.c_int),))
    with pytest.raises(AttributeError, match="mcq_no_such_entry"):
        _lib.load_library()
    assert _lib._lib is None


LAW = "law must be 'reference' or 'uniform'"
PER_QUERY = "one mcq_query_ext per query"


def test_argument_errors_come_before_the_engine():
    """Every ValueError below is raised with None in place of the engine: nothing of it was touched."""
    E, M = npa.Engine, npa.MultiEngine
    q = _lib.pack_query_one([0, 5], [4, 17, 22], 2, 1)
    x = _lib.pack_query_ext(1)
    xx = np.concatenate([x, x])
    with_law = (E.exact_ext, E.exact_ext_ways, E.exact_ext_runouts, E.exact_seats, E.exact_ext_seats, E.exact_hero_range,
                E.exact_hero_range_preflop)
    cases = [(E.exact, (q,), {"law": "x"}, LAW)]
    cases += [(f, (q, x), {"law": "x"}, LAW) for f in with_law]
    cases += [(f, (q, xx), {"law": "x"}, LAW) for f in with_law]            # two faults: the law is checked first
    cases += [(f, (q, xx), {}, PER_QUERY) for f in with_law]
    cases += [(f, (q, xx, 0), {}, PER_QUERY) for f in (E.eval_batch_ext, E.eval_batch_ext_ways, E.eval_batch_ext_seats)]
    cases += [
        (E.eval_batch, (q, 0), {"mode": _lib.MODE_REPLAY_MT19937, "part": (0, 2)},
         "only the production mode can split the iterations of a query"),
        (E.exact_matrix, (np.zeros(0, _lib.MATRIX_QUERY_DTYPE),), {}, "1 to MATRIX_MAX_BATCH = 256 records per call"),
        (E.showdown, (np.zeros((2, 3, 6), np.uint8),), {}, "hands must have shape [tables, players, 7]"),
        (E.eval_batch_ranges, (q, np.zeros((1, 10), np.uint32), np.ones((1, 1325), np.uint16), 0), {},
         "tables is a uint16 array of shape [n_tables >= 1, HAND_ROWS = 1326]"),
        (E.eval_batch_ranges, (q, np.zeros((2, 10), np.uint32), np.ones((1, 1326), np.uint16), 0), {},
         "seat_table is a uint32 array of shape [n, 10] = (1, 10)"),
        (E.eval_batch_ranges, (q, np.zeros((2, 10), np.uint32), np.ones((1, 1325), np.uint16), 0), {},   # tables first
         "tables is a uint16 array of shape [n_tables >= 1, HAND_ROWS = 1326]"),
        (E.set_dealing_law, ("x",), {}, LAW),
        (M.set_dealing_law, ("x",), {}, LAW),
        (M.eval_batch, (q, 0), {"partition": "x"}, "partition must be 'auto', 'queries' or 'iterations'"),
    ]
    for f, args, kwargs, text in cases:
        with pytest.raises(ValueError) as err:
            f(None, *args, **kwargs)
        assert text in str(err.value), (f.__name__, str(err.value))


def test_return_codes_map_to_the_same_exceptions():
    assert (_lib.MCQ_EINVAL, _lib.MCQ_EDEVICE, _lib.MCQ_ENOMEM, _lib.MCQ_EBUSY) == (-1, -2, -3, -4)
    with pytest.raises(ValueError):
        _lib._raise(_lib.MCQ_EINVAL)
    with pytest.raises(npa.McqBusyError):
        _lib._raise(_lib.MCQ_EBUSY)
    for rc in (_lib.MCQ_EDEVICE, _lib.MCQ_ENOMEM):
        with pytest.raises(npa.McqError) as err:
            _lib._raise(rc)
        assert type(err.value) is npa.McqError and str(err.value).startswith("libmcq_hip error %d" % rc)
    # the call helper of the engine classes: a zero return passes, anything else goes through _raise
    assert _lib._call(lambda *a: 0, 1, 2) is None
    with pytest.raises(npa.McqBusyError):
        _lib._call(lambda *a: _lib.MCQ_EBUSY)


def test_an_error_under_the_bindings_lock_is_raised():
    """set_default_dealing_law and default_engine call into engines while they hold _lib._lock; an engine in the middle of
    a call answers MCQ_EBUSY there, and raising it must not wait for that lock (once the library is loaded)."""
    npa.load_library()
    assert _lib._lock.acquire(timeout=5)
    try:
        with pytest.raises(npa.McqBusyError):
            _lib._raise(_lib.MCQ_EBUSY)
    finally:
        _lib._lock.release()
