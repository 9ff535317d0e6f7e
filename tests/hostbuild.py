"""The one place where the host builds of the lane code (tests/hostsim*) are compiled, loaded and, as stand-alone
programs, run under the host sanitizers; and the record coercions those packages share.  A path that is not absolute
is taken from this directory, so nothing depends on the working directory."""
import ctypes
import os
import subprocess

import numpy as np

_TESTS = os.path.dirname(os.path.abspath(__file__))
_WARN = ["-std=c++17", "-pthread", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized"]
_loaded = {}


def _stale(so):
    """Missing, no dependency file beside it, or older than a file the compiler read for it (`so`.d, written by -MMD)."""
    try:
        built = os.path.getmtime(so)
        deps = open(so + ".d").read().replace("\\\n", " ").split(": ", 1)[1].split()
        return not deps or any(os.path.getmtime(d) > built for d in deps)
    except (OSError, IndexError):
        return True


def load(cpp, so=None, env=None):
    """Shared library of the one translation unit `cpp` -> ctypes.CDLL, built first when stale.  `so` defaults to
    lib<name>.so beside the source.  With the environment variable `env` set, the file it names is loaded as it is."""
    cpp = os.path.join(_TESTS, cpp)
    so = os.path.join(_TESTS, so) if so else os.path.join(os.path.dirname(cpp), "lib%s.so" % os.path.basename(cpp)[:-4])
    override = os.environ.get(env) if env else None
    path = override or so
    if path not in _loaded:
        if not override and _stale(so):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            try:
                subprocess.check_call(["g++", "-O2", *_WARN, "-shared", "-fPIC", "-MMD", "-MF", tmp + ".d", "-o", tmp, cpp])
                os.replace(tmp + ".d", so + ".d")       # first: an old library beside new dependencies is still stale
                os.replace(tmp, so)
            finally:
                for left in (tmp, tmp + ".d"):
                    if os.path.exists(left):
                        os.remove(left)
        _loaded[path] = ctypes.CDLL(path)
    return _loaded[path]


def run_sanitized(cpp, opt, tmp_path):
    """Build the program `cpp` (it has a main) at optimisation level `opt` with AddressSanitizer and
    UndefinedBehaviorSanitizer into tmp_path, run it as a process of its own -> its output lines."""
    exe = os.path.join(str(tmp_path), os.path.basename(cpp)[:-4])
    subprocess.check_call(["g++", opt, "-g", *_WARN, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(_TESTS, cpp), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return res.stdout.strip().splitlines()


def first_bytes(a, n):
    """The first n bytes of an array or record as a fresh contiguous uint8 array."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:n].copy()


def record(query16, ext):
    """(the query's 16 bytes, the extension's 304 bytes)"""
    return first_bytes(query16, 16), first_bytes(ext, 304)


def rows(entry, queries, width, *args, qid_at=None):
    """One 16-byte record of `queries` at a time through entry(record, *args, row) -> uint64 [n, width].  qid_at: the
    place in args of the first query's id; query i gets that id + i.  ValueError on a return other than 0."""
    q = np.ascontiguousarray(queries).view(np.uint8).reshape(-1, 16)
    out = np.zeros((len(q), width), np.uint64)
    for i in range(len(q)):
        rec = q[i].copy()
        a = [v + i if k == qid_at else v for k, v in enumerate(args)]
        rc = entry(rec.ctypes.data_as(ctypes.c_void_p), *a, out[i].ctypes.data_as(ctypes.c_void_p))
        if rc:
            raise ValueError("%s: %d (arguments %s, query %s)" % (entry.__name__, rc, a, rec.tolist()))
    return out
