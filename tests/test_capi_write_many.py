"""ez_writer_write_many at the drop-in boundary: both entry points exported and declared, the
empty call without a device (CPU), and the C++ mirror's WriteMany against Write (GPU)."""

import ctypes as C
import os
import subprocess

import pytest

import eazy_amd as ez

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
NAMES = ("ez_writer_write_many", "ez_writer_write_many_last")


def test_write_many_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", ez.LIB_PATH], capture_output=True, text=True).stdout
    hdr = open(os.path.join(ROOT, "include", "eazy.h")).read()
    for n in NAMES:
        assert f" T {n}\n" in out, n
        assert f"int {n}(" in hdr and n in ez.exported_symbols(), n
    assert '"hm:lds"' in hdr and '"hm:lds+own"' in hdr and '"hm:own"' in hdr  # ez_compress_route_last names the routes


def test_write_many_of_nothing_needs_no_device():
    L = ez._lib()
    L.ez_writer_write_many.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert L.ez_writer_write_many(None, 0, None, None, None, 0, None, None) == ez.OK
    counts = (C.c_uint64 * 2)(7, 7)
    assert L.ez_writer_write_many_last(counts) == ez.OK and list(counts) == [0, 0]
    assert ez.write_many([], []) == []
    with pytest.raises(ValueError):
        ez.write_many([], [b"x"])


def _build():
    """tests/cpp/write_many_test, compiled as tests/cpp/Makefile compiles eazy_test (when older than its sources)."""
    exe, src = os.path.join(CPP, "write_many_test"), os.path.join(CPP, "write_many_test.cpp")
    deps = [src, os.path.join(ROOT, "eazy_amd", "cpp", "eazy.hpp"), os.path.join(ROOT, "include", "eazy.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "eazy_amd")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-o", exe, src, f"-L{libdir}", "-leazy_amd", f"-Wl,-rpath,{libdir}"],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_cpp_write_many_compiles():
    _build()


@pytest.mark.gpu
def test_cpp_write_many(cuda):
    """4 Writers through WriteMany for three rounds against 4 through Write: the same sink calls."""
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "write_many ok" in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
