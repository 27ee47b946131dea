"""The K2r decoder's per-lane code (eazy_amd/csrc/ez_decompress_ring.hip),
compiled for the host by tools/ring_emu.hip and run stream by stream on the
oracle's compressed streams: the decoded bytes must be the original input.
CPU only — it checks the kernel's logic (LDS ring indexing, mirror, whole-line
flushes, zero history) here; the GPU tests run the same code on the MI355X.

The second half runs the hand-built streams of the K2r suite (tests/k2r_streams.py; the GPU half is
tests/test_gpu_k2r.py) raw: the bytes must equal the oracle's, and the streams the lane code hands
over (size ~0) must be exactly the ones the oracle gives an error for or that do not fit their
slot.  The output buffer starts as 0xA5 bytes, so the zero history is not the buffer's own zeros."""

import os
import subprocess

import numpy as np
import pytest

import k2r_streams as k2r
import oracle as orc
from k2_streams import _need, _oracle, _slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "ring_emu")


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tools", "ring_emu.hip")
    deps = [src] + [os.path.join(ROOT, "eazy_amd", "csrc", f) for f in ("ez_decompress_ring.hip", "ez_k2_parse.h", "ez_bytes.h", "ez_format.h",
                                                                              "ez_internal.h")]
    if not os.path.exists(EMU) or os.path.getmtime(EMU) < max(os.path.getmtime(d) for d in deps):
        p = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-align-mismatch",
                            "-o", EMU, src], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    return EMU


@pytest.fixture(params=[1, 0], ids=["header-window", "header-per-token"])
def hw(request):
    return request.param


def _run(emu, tmp_path, bufs, block=1 << 20, htable=1024, hw=1):
    comp = [orc.compress(block, htable, [b]) for b in bufs]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in comp])]).astype(np.uint64)
    cap = max(16, max(len(b) for b in bufs))
    (tmp_path / "in").write_bytes(b"".join(comp))
    (tmp_path / "off").write_bytes(offs.tobytes())
    subprocess.run([emu, str(tmp_path / "in"), str(tmp_path / "off"), str(cap), str(tmp_path / "out"), str(tmp_path / "sz"), str(hw)],
                   check=True, timeout=600)
    out = (tmp_path / "out").read_bytes()
    sz = np.frombuffer((tmp_path / "sz").read_bytes(), np.uint64)
    at = 0
    for s, b in enumerate(bufs):
        assert sz[s] != np.uint64(~np.uint64(0)), f"stream {s} (len {len(b)}) handed over"
        assert out[at : at + int(sz[s])] == b, f"stream {s} (len {len(b)})"
        at += int(sz[s])


def test_logs(emu, tmp_path, hw):
    from eazy_amd import synth

    d = synth.logs(3, 256 * 4096).tobytes()
    _run(emu, tmp_path, [d[k * 4096 : (k + 1) * 4096] for k in range(256)], hw=hw)


def test_long_streams(emu, tmp_path, hw):
    """Streams much longer than the ring: far copies read the flushed output."""
    from eazy_amd import synth

    d = synth.logs(5, 4 << 20).tobytes()
    _run(emu, tmp_path, [d[: 1 << 20], d[1 << 20 : (1 << 20) + 100003], d[3 << 20 :]], hw=hw)


def test_edges_random_runs(emu, tmp_path, hw):
    from eazy_amd import synth

    rng = np.random.default_rng(11)
    d = synth.logs(9, 1 << 20).tobytes()
    bufs = [b"", b"a", b"abcd", b"aaaaaaaaaaaa", bytes(64), bytes(7), bytes(9), bytes(17), b"ab" * 40, bytes(1000), b"xyz" * 700]
    at = 0
    for n in rng.integers(0, 9000, 40):
        bufs.append(d[at : at + int(n)])
        at += int(n)
    for k in range(24):
        n = int(rng.integers(100, 20000))
        kind = k % 4
        if kind == 0:
            b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            b = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
        elif kind == 2:
            b = (bytes(rng.integers(0, 256, 7, dtype=np.uint8)) * (n // 7 + 1))[:n]
        else:
            z = np.zeros(n, np.uint8)
            idx = rng.integers(0, n, n // 10)
            z[idx] = rng.integers(1, 256, len(idx), dtype=np.uint8)
            b = z.tobytes()
        bufs.append(b)
    _run(emu, tmp_path, bufs, hw=hw)


# ---------------------------------------------------------------- hand-built streams (tests/k2r_streams.py)


def _run_raw(emu, tmp_path, cases, hw=1, limit=0, handed="auto"):
    """The raw streams of `cases` as one batch through the lane code, each in its own slot (the
    case's, or the oracle's length plus 1..5 bytes and at least 16): bytes equal the oracle's, and
    the handed-over set is the expected one."""
    ins = [c.stream for c in cases]
    caps = [c.slot if c.slot is not None else max(16, _slot(s, _need(c.stream, limit))) for s, c in enumerate(cases)]
    offs = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.uint64)
    (tmp_path / "in").write_bytes(b"".join(ins))
    (tmp_path / "off").write_bytes(offs.tobytes())
    (tmp_path / "caps").write_bytes(np.asarray(caps, np.uint64).tobytes())
    subprocess.run([emu, str(tmp_path / "in"), str(tmp_path / "off"), "0", str(tmp_path / "out"), str(tmp_path / "sz"), str(hw), str(limit),
                    str(tmp_path / "caps")], check=True, timeout=600, stderr=subprocess.DEVNULL)
    out = (tmp_path / "out").read_bytes()
    sz = np.frombuffer((tmp_path / "sz").read_bytes(), np.uint64)
    gone = np.uint64(~np.uint64(0))
    expect = k2r.expected_handed([c._replace(slot=caps[s]) for s, c in enumerate(cases)], limit) if handed == "auto" else set(handed)
    got = {s for s in range(len(cases)) if sz[s] == gone}
    assert got == expect, ([cases[s].name for s in sorted(got ^ expect)][:8], len(got), len(expect))
    at = 0
    for s, c in enumerate(cases):
        if sz[s] == gone:
            continue
        want, err = _oracle(c.stream, caps[s], limit)
        assert err == 0 and out[at : at + int(sz[s])] == want, c.name
        at += int(sz[s])
    assert at == len(out)


@pytest.mark.parametrize("group", ["r1", "r2", "r3", "r4", "r5", "r6"])
def test_hand_built(emu, tmp_path, hw, group):
    """R1 the ring / HBM threshold, R2 ring residues, R3 runs and zero regions, R4 literal + copy
    pairs, R5 slot edges (k2r_streams): only the streams with an error or a slot too small are
    handed over."""
    cases = getattr(k2r, group + "_streams")()
    if group not in ("r5", "r6"):  # (the groups' valid streams: every one but the named error cases)
        for c in cases:
            if c.slot is None and "window-D1025" not in c.name:
                assert _oracle(c.stream, 1 << 20)[1] == 0, c.name
    _run_raw(emu, tmp_path, cases, hw=hw)


def test_hand_built_block_size_limit(emu, tmp_path, hw):
    """R4 with BlockSizeLimit = 8: L1 and L2 at the limit decode, one more is handed over."""
    cases = k2r.r4_limit_streams()
    bad = k2r.expected_handed(cases, k2r.R4_LIMIT)
    for s, c in enumerate(cases):
        assert (s in bad) == ("L1_9" in c.name or "L1_10" in c.name or "L2_9" in c.name or "D9" in c.name), c.name
    _run_raw(emu, tmp_path, cases, hw=hw, limit=k2r.R4_LIMIT)


def test_hand_built_last_streams(emu, tmp_path, hw):
    """R5: the last stream of a batch ends in a literal of 1..20, 31, 32, 33 bytes, in a copy header,
    or is shorter than 16 bytes in all: loads are clamped to the batch's last 16 bytes."""
    for name, cases in k2r.r5_last_stream_batches():
        d = tmp_path / name
        d.mkdir()
        _run_raw(emu, d, cases, hw=hw)
