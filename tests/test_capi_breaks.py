"""The Break index's C entry points (include/eazy.h: ez_breaks_workspace, ez_stream_breaks_batch):
declared, exported, bound by the Python mirror, the header still C99, the refusals, and no CPU
fallback.  CPU only."""

import ctypes as C
import os
import subprocess

import pytest

import eazy_amd as ez

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ez_breaks_workspace", "ez_stream_breaks_batch")


def test_breaks_symbols_declared_exported_and_bound():
    lib = ez._lib()
    declared = ez.exported_symbols()
    hdr = open(os.path.join(ROOT, "include", "eazy.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", ez.LIB_PATH], capture_output=True, text=True).stdout
    for n in NAMES:
        assert n in declared and f" {n}(" in hdr, n
        assert f" T {n}\n" in out, n
        assert getattr(lib, n).argtypes is not None, n  # (bound with its argument types, not looked up by default)
    assert lib.ez_abi_version() == 2  # additions only
    assert callable(ez.stream_breaks)


def test_header_still_compiles_as_c99():
    src = os.path.join(ROOT, "include", "eazy.h")
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_workspace_size_is_a_host_function():
    L = ez._lib()
    sizes = [L.ez_breaks_workspace(n) for n in (0, 1, 2, 63, 64, 1000, 65536)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert all(s % 16 == 0 for s in sizes)


def _args():
    """Host arrays standing in for device ones: the refusals and the device check come before any use."""
    words = (C.c_uint64 * 8)()
    p = C.addressof(words)
    return words, ez._Batch(p, p, None, None, p, p, 1, 0, 0, 0), p


def test_refusals_come_before_any_device_use():
    L = ez._lib()
    words, b, p = _args()
    assert L.ez_stream_breaks_batch(0, None, p, p, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), None, p, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), p, None, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), p, p, 4, None, None, None) == ez.EINVAL
    nb = ez._Batch(p, p, None, None, None, p, 1, 0, 0, 0)
    assert L.ez_stream_breaks_batch(0, C.byref(nb), p, p, 4, p, None, None) == ez.EINVAL
    assert list(words) == [0] * 8


def test_break_query_needs_a_device():
    if ez.device_count() > 0:
        pytest.skip("GPU present")
    words, b, p = _args()
    assert ez._lib().ez_stream_breaks_batch(0, C.byref(b), p, p, 4, p, None, None) == ez.EDEVICE
    assert ez._lib().ez_stream_breaks_batch(0, C.byref(b), p, None, 0, p, None, None) == ez.EDEVICE
    assert list(words) == [0] * 8
