"""tests/hostbuild.py, the loader of the host builds: what makes a library stale is the compiler's own list of the files
it read, the override variable loads a file as it is, and a build leaves nothing but the library and its dependency file."""
import os
import subprocess
import sys
import time

import pytest

from tests import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, **env):
    """A fresh interpreter (a process loads each path once) -> what it printed"""
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), check=True,
                          stdout=subprocess.PIPE, text=True).stdout.strip()


def _value(cpp):
    return int(_child("from tests import hostbuild; print(hostbuild.load(%r).hb_value())" % cpp))


def _touch_past(path, other):
    t = os.path.getmtime(other) + 1
    os.utime(path, (t, t))


@pytest.fixture
def tree(tmp_path):
    """a.cpp includes b.hpp includes c.hpp, d.hpp lies beside them; built once, and every file dated well before now:
    the sources 200 s ago, the library 100 s ago"""
    (tmp_path / "a.cpp").write_text('#include "b.hpp"\nextern "C" int hb_value() { return HB_VALUE; }\n')
    (tmp_path / "b.hpp").write_text('#include "c.hpp"\n')
    (tmp_path / "c.hpp").write_text("#define HB_VALUE 41\n")
    (tmp_path / "d.hpp").write_text("#define HB_VALUE 13\n")
    cpp, so = str(tmp_path / "a.cpp"), str(tmp_path / "liba.so")
    assert hostbuild.load(cpp).hb_value() == 41                       # the first call builds
    assert hostbuild.load(cpp) is hostbuild.load(cpp)                 # ... and the process keeps the handle
    assert sorted(os.listdir(tmp_path)) == ["a.cpp", "b.hpp", "c.hpp", "d.hpp", "liba.so", "liba.so.d"]   # no temporary left
    now = time.time()
    for name in os.listdir(tmp_path):
        t = now - (100 if name.startswith("liba.so") else 200)
        os.utime(str(tmp_path / name), (t, t))
    return cpp, so


def test_a_second_load_does_not_rebuild(tree):
    cpp, so = tree
    built = os.path.getmtime(so)
    assert _value(cpp) == 41 and os.path.getmtime(so) == built


def test_a_newer_header_two_includes_away_rebuilds(tree):
    cpp, so = tree
    built = os.path.getmtime(so)
    with open(os.path.join(os.path.dirname(cpp), "c.hpp"), "w") as f:
        f.write("#define HB_VALUE 42\n")
    _touch_past(os.path.join(os.path.dirname(cpp), "c.hpp"), so)
    assert _value(cpp) == 42 and os.path.getmtime(so) > built
    assert not [n for n in os.listdir(os.path.dirname(cpp)) if ".tmp" in n]
    rebuilt = os.path.getmtime(so)
    assert _value(cpp) == 42 and os.path.getmtime(so) == rebuilt      # and is fresh again


def test_a_newer_file_that_is_not_included_does_not(tree):
    cpp, so = tree
    built = os.path.getmtime(so)
    _touch_past(os.path.join(os.path.dirname(cpp), "d.hpp"), so)
    assert _value(cpp) == 41 and os.path.getmtime(so) == built


def test_without_its_dependency_file_a_library_is_stale(tree):
    cpp, so = tree
    built = os.path.getmtime(so)
    os.remove(so + ".d")
    assert _value(cpp) == 41 and os.path.getmtime(so) > built and os.path.exists(so + ".d")


def test_the_override_variable_loads_the_named_file_as_it_is(tmp_path):
    """MCQ_HOSTSIM_SO (tests/sanitize_cpu.sh sets it): tests.hostsim loads that file and neither builds nor checks its own."""
    mine = str(tmp_path / "libelsewhere.so")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-pthread", "-shared", "-fPIC", "-o", mine,
                           os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")])
    own = os.path.join(ROOT, "tests", "hostsim", "libmcq_hostsim.so")
    before = os.path.getmtime(own) if os.path.exists(own) else None
    assert _child("from tests import hostsim; print(hostsim.lib()._name)", MCQ_HOSTSIM_SO=mine) == mine
    assert (os.path.getmtime(own) if os.path.exists(own) else None) == before
