"""The C++ mirror of the Break index (eazy::StreamBreaksBatch, eazy_amd/cpp/eazy.hpp):
tests/cpp/breaks_test.cpp builds 16 streams of messages with a Break behind each, checks the query's
positions with and without a workspace and with too little room, and splits the segmented decode's
output at them; compiled as tests/cpp/Makefile compiles eazy_test."""

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")


def _build():
    exe, src = os.path.join(CPP, "breaks_test"), os.path.join(CPP, "breaks_test.cpp")
    deps = [src, os.path.join(ROOT, "eazy_amd", "cpp", "eazy.hpp"), os.path.join(ROOT, "include", "eazy.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "eazy_amd")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-o", exe, src, f"-L{libdir}", "-leazy_amd", f"-Wl,-rpath,{libdir}"],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_cpp_breaks_compiles():
    _build()


@pytest.mark.gpu
def test_cpp_breaks_round_trip(cuda):
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "breaks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
