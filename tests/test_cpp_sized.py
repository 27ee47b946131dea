"""The C++ mirror of the sized decode (eazy::DecompressedSizeSegsLast and eazy::DecompressBatchSized,
eazy_amd/cpp/eazy.hpp): tests/cpp/sized_test.cpp sizes 64 streams of 4 joined streams each, reads the
size query's K2g counters, decodes through the segmented route and gets the plain bytes back, then
does the same with the 256 streams on their own, which take DecompressBatch's decoders; compiled as
tests/cpp/Makefile compiles eazy_test."""

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")


def _build():
    exe, src = os.path.join(CPP, "sized_test"), os.path.join(CPP, "sized_test.cpp")
    deps = [src, os.path.join(ROOT, "eazy_amd", "cpp", "eazy.hpp"), os.path.join(ROOT, "include", "eazy.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "eazy_amd")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-o", exe, src, f"-L{libdir}", "-leazy_amd", f"-Wl,-rpath,{libdir}"],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_cpp_sized_compiles():
    _build()


@pytest.mark.gpu
def test_cpp_sized_round_trip(cuda):
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "sized ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
