"""The decoded-size query's C entry points (include/eazy.h: ez_decompressed_size_batch,
ez_decompressed_size_chunk, ez_decompressed_size_chunk_last): exported, the chunk choice a plain host
function, and no CPU fallback.  CPU only."""

import subprocess

import pytest

import eazy_amd as ez

NAMES = ("ez_decompressed_size_batch", "ez_decompressed_size_chunk", "ez_decompressed_size_chunk_last")


def test_size_symbols_exported():
    lib = ez._lib()
    declared = ez.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", ez.LIB_PATH], capture_output=True, text=True).stdout
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert f" T {n}\n" in out, n
    assert lib.ez_abi_version() == 2  # ez_batch is unchanged


def test_chunk_is_a_monotone_power_of_two():
    # hint 0 means unknown; over the known hints the chunk never shrinks as the hint grows
    hints = [1, 2, 63, 64, 65, 1000, 2048, 4095, 4096, 4097, 8192, 65536, 1 << 20, 1 << 22, 1 << 31, 1 << 40, (1 << 64) - 1]
    got = [ez.decompressed_size_chunk(h) for h in [0] + hints]
    for c in got:
        assert 32 <= c <= 1024 and c & (c - 1) == 0, got
    known = got[1:]
    assert known == sorted(known), known
    assert ez.decompressed_size_chunk(0) in known  # unknown: one of the known hints' chunks


def test_size_query_needs_a_device():
    if ez.device_count() > 0:
        pytest.skip("GPU present")
    assert ez._lib().ez_decompressed_size_batch(0, None, None, None) == ez.EDEVICE
