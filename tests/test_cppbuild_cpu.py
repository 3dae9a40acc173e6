"""CPU tier: the routine every test compiles C++ with (tests/cppbuild.py): it rebuilds what is stale and only that, a compile that
fails leaves the previous output whole, the VAR_ slots of a run-time scene are numbered by first appearance, and a host render takes
16 threads at the most."""
import ctypes
import os
import subprocess

import pytest

import cppbuild

SOURCE = """
extern "C" int answer() { return 42; }
"""


def _later(path, than):
    t = os.path.getmtime(than) + 10
    os.utime(path, (t, t))


def test_compile_rebuilds_what_is_stale_and_keeps_the_output_of_a_failed_compile(tmp_path, capfd):
    src, dep, so = str(tmp_path / "answer.cpp"), str(tmp_path / "answer.h"), str(tmp_path / "out" / "libanswer.so")
    for path, text in ((src, SOURCE), (dep, "")):
        with open(path, "w") as f:
            f.write(text)
    assert cppbuild.compile(so, [src], [dep], ["-fPIC"]) == so  # makes the directory
    # (a) fresh: not rebuilt
    os.utime(so, (1e9, 1e9))
    os.utime(src, (1e9 - 10, 1e9 - 10))
    os.utime(dep, (1e9 - 10, 1e9 - 10))
    cppbuild.compile(so, [src], [dep], ["-fPIC"])
    assert os.path.getmtime(so) == 1e9
    # (b) a newer dependency: rebuilt
    _later(dep, so)
    cppbuild.compile(so, [src], [dep], ["-fPIC"])
    assert os.path.getmtime(so) > os.path.getmtime(dep)
    # (c) a source that does not compile: raises, and the previous output is what it was
    before = open(so, "rb").read()
    with open(src, "w") as f:
        f.write("this is not C++\n")
    _later(src, so)
    with pytest.raises(subprocess.CalledProcessError):
        cppbuild.compile(so, [src], [dep], ["-fPIC"])
    capfd.readouterr()  # the compiler's complaint
    assert open(so, "rb").read() == before and os.listdir(os.path.dirname(so)) == ["libanswer.so"]
    assert ctypes.CDLL(so).answer() == 42  # (the first load of this path in the process)


def test_scene_include_numbers_the_slots_by_first_appearance(tmp_path):
    path = str(tmp_path / "gen" / "s.scene.inc")
    text = "float map() { return VAR_b(1, 0, 2) + VAR_a (0.5) * VAR_b(1, 0, 2); }\n"
    assert cppbuild.scene_include(path, text) == ["b", "a"]
    assert open(path).read() == "#define VAR_b(...) (U.scene_var[0])\n#define VAR_a(...) (U.scene_var[1])\n" + text
    assert cppbuild.scene_include(path, text, str.upper) == ["b", "a"]
    assert open(path).read().endswith("#define VAR_a(...) (U.scene_var[1])\n" + text.upper())
    # unchanged text: the file is not written again
    os.utime(path, (1e9, 1e9))
    cppbuild.scene_include(path, text, str.upper)
    assert os.path.getmtime(path) == 1e9


def test_default_threads_is_16_at_the_most():
    assert 1 <= cppbuild.default_threads() <= 16
