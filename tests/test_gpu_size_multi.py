"""ez_decompressed_size_batch_multi, the host-memory twin of the decoded-size query: exported,
declared and refusing NULL arrays without a device (CPU); over one shard and over two shards of
device 0 equal to the device query on a ragged batch with empty streams and error streams, the sized
multi-device decode equal to the sized device decode, and the C++ mirror (tests/cpp/size_multi_test.cpp)
(GPU)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eazy_amd as ez

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
ARGS = [C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]


def test_symbol_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", ez.LIB_PATH], capture_output=True, text=True).stdout
    hdr = open(os.path.join(ROOT, "include", "eazy.h")).read()
    for n in ("ez_decompressed_size_batch_multi", "ez_reader_whole_slot", "ez_reader_whole_launches"):
        assert f" T {n}\n" in out, n
        assert f"{n}(" in hdr and n in ez.exported_symbols(), n


def test_refuses_null_arrays_without_a_device():
    L = ez._lib()
    L.ez_decompressed_size_batch_multi.argtypes = ARGS
    off = (C.c_uint64 * 2)(0, 0)
    size = (C.c_uint64 * 1)(7)
    assert L.ez_decompressed_size_batch_multi(0, None, None, 1, None, 0, size, None) == ez.EINVAL
    assert L.ez_decompressed_size_batch_multi(0, None, off, 1, None, 0, None, None) == ez.EINVAL
    assert L.ez_decompressed_size_batch_multi(0, None, None, 0, None, 0, None, None) == ez.EINVAL
    assert size[0] == 7
    if ez.device_count() <= 0:
        assert L.ez_decompressed_size_batch_multi(0, None, off, 0, None, 0, size, None) == ez.EDEVICE
    else:
        assert L.ez_decompressed_size_batch_multi(0, None, off, 0, None, 0, size, None) == ez.OK  # count == 0


def _build():
    """tests/cpp/size_multi_test, compiled as tests/cpp/Makefile compiles eazy_test (when older than its sources)."""
    exe, src = os.path.join(CPP, "size_multi_test"), os.path.join(CPP, "size_multi_test.cpp")
    deps = [src, os.path.join(ROOT, "eazy_amd", "cpp", "eazy.hpp"), os.path.join(ROOT, "include", "eazy.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "eazy_amd")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-o", exe, src, f"-L{libdir}", "-leazy_amd", f"-Wl,-rpath,{libdir}"],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_cpp_size_multi_compiles():
    _build()


def _ragged():
    """Compressed log streams of ragged lengths with empty streams, a header-only one, a truncated one,
    one with a distance past its window and one with a MetaReset after output between them."""
    from eazy_amd import synth
    from k2_streams import HDR, HDR_1K, META_RESET, cpy, lit, meta

    import oracle as orc

    lens = [70000, 0, 300, 1 << 20, 4096, 0, 250001, 17]
    host = synth.logs(17, sum(lens))
    plain, at = [], 0
    for n in lens:
        plain.append(host[at : at + n].tobytes())
        at += n
    ins = [orc.compress(ez.MiB, 1024, [p]) if p else b"" for p in plain]
    extra = [HDR, ins[3][: len(ins[3]) - 9], HDR_1K + lit(bytes(2000)) + cpy(1500, 20) + lit(b"q"),
             HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b"), b""]
    return ins[:4] + extra[:3] + ins[4:] + extra[3:]


@pytest.mark.gpu
def test_sizes_multi_equal_the_device_query(cuda):
    import torch

    ins = _ragged()
    off = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    comp = np.frombuffer(b"".join(ins), np.uint8)
    d_sz, d_st = ez.decompressed_sizes(torch.from_numpy(comp.copy()).to(cuda), torch.from_numpy(off).to(cuda))
    torch.cuda.synchronize()
    d_sz, d_st = d_sz.cpu().numpy(), d_st.cpu().numpy()
    assert (d_st != 0).sum() >= 2 and (d_st == 0).sum() >= 8  # (errors and clean streams both present)
    for devs in ([0], [0, 0]):
        sz, st = ez.decompressed_sizes_multi(comp, off, devices=devs)
        assert np.array_equal(sz, d_sz) and np.array_equal(st, d_st), devs
    assert ez.decompressed_sizes_multi(b"", np.array([0]), devices=[0])[0].size == 0


@pytest.mark.gpu
def test_sized_multi_decode_equals_the_sized_device_decode(cuda):
    import torch

    ins = _ragged()
    off = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    comp = np.frombuffer(b"".join(ins), np.uint8)
    out, out_off, sizes, status = ez.decompress_batch_sized(torch.from_numpy(comp.copy()).to(cuda), torch.from_numpy(off).to(cuda))
    torch.cuda.synchronize()
    out, out_off, sizes, status = out.cpu().numpy(), out_off.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy()
    for devs in ([0], [0, 0]):
        m_out, m_off, m_sizes, m_status = ez.decompress_batch_multi_sized(comp, off, devices=devs)
        assert np.array_equal(m_off, out_off) and np.array_equal(m_sizes, sizes) and np.array_equal(m_status, status), devs
        for s in range(len(ins)):
            a = int(out_off[s])
            if status[s] == 0:
                assert m_out[a : a + int(sizes[s])].tobytes() == out[a : a + int(sizes[s])].tobytes(), (devs, s)


@pytest.mark.gpu
def test_cpp_size_multi(cuda):
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "size_multi ok" in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
