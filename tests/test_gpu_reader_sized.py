"""A NewReaderBytes handle sizes its whole-stream slot from the decoded-size query (reader_ahead,
eazy_amd/csrc/ez_reader.hip): one decode into a slot of the stream's exact size, or none at all where
the query gives an error or a size over 1 GiB.  Every Read's bytes and error equal the oracle's
Reader's, and ez_reader_whole_slot / ez_reader_whole_launches say what the first Read did:
a stream that expands more than 8 x (two decodes before: the first slot was 8 x the input),
256 KiB of incompressible bytes (a slot of 8 x the input before), a stream with Breaks, and the
bomb and a truncated stream (no decode, no slot: the same errors at the same Reads as a handle that
decodes Read by Read)."""

import numpy as np
import pytest

import impls
import oracle as orc
from k2_streams import HDR, cpy, lit

pytestmark = pytest.mark.gpu


def _stream(parts, brk=()):
    w = orc.Writer(1 << 20, 1024)
    for k, p in enumerate(parts):
        for _ in range(brk.count(k)):
            assert w.write_break() == 0
        assert w.write(p) == (len(p), 0)
    return bytes(w.sink)


def _reads(r, size, most):
    """Up to `most` Reads of `size` bytes -> [(bytes, error)], ending at the first error that is not a Break."""
    import eazy_amd as ez

    out = []
    for _ in range(most):
        got, err = r.read(size)
        out.append((bytes(got), err))
        if err not in (ez.OK, ez.EBREAK):
            break
    return out


def _check(b, size, most=100000):
    """The handle's Reads against the oracle's; returns (the handle, the output's length)."""
    G = impls.Gpu()
    rb = G.Rb(b)
    got = _reads(rb, size, most)
    want = _reads(orc.Reader(b=b), size, most)
    assert [e for _, e in got] == [e for _, e in want], (size, [e for _, e in got][-3:], [e for _, e in want][-3:])
    assert got == want, size
    return rb, sum(len(g) for g, _ in got)


def test_ratio_above_8_decodes_once(cuda):
    parts = [bytes(1 << 18) + bytes([k + 1]) * 64 for k in range(8)]
    b = _stream(parts)
    out = b"".join(parts)
    assert orc.decompress(b, cap=len(out) + 16)[0] == out and len(out) > 8 * len(b) + 4096
    for size in (4096, 1 << 20):
        rb, n = _check(b, size)
        assert n == len(out) and rb.r.whole_decoded
        assert rb.r.whole_launches == 1
        assert 0 <= rb.r.whole_slot - ((len(out) + 15) & ~15) <= 64, rb.r.whole_slot


def test_incompressible_slot_is_not_8x(cuda):
    rng = np.random.default_rng(401)
    plain = rng.integers(0, 256, 256 << 10, dtype=np.uint8).tobytes()
    b = _stream([plain])
    rb, n = _check(b, 65536)
    assert n == len(plain) and rb.r.whole_decoded and rb.r.whole_launches == 1
    assert len(plain) <= rb.r.whole_slot < 2 * len(plain), rb.r.whole_slot


def test_breaks(cuda):
    import eazy_amd as ez
    from eazy_amd import synth

    plain = synth.logs(91, 1 << 20).tobytes()
    chunks = [plain[k : k + 100_000] for k in range(0, len(plain), 100_000)]
    b = _stream(chunks, brk=(0, 3, 3, 7, len(chunks) - 1))
    for size in (4096, 300_000):
        rb, n = _check(b, size)
        assert n == len(plain) and rb.r.whole_decoded and rb.r.whole_launches == 1
        assert 0 <= rb.r.whole_slot - ((len(plain) + 15) & ~15) <= 64
    G = impls.Gpu()
    assert [e for _, e in _reads(G.Rb(b), 4096, 100000)].count(ez.EBREAK) == 5


def test_bomb_and_error_decode_nothing_whole(cuda):
    import eazy_amd as ez
    from eazy_amd import synth

    bomb = HDR + lit(b"x") + cpy(1, 1 << 29) * 20  # over 10 GiB: 16 Reads of it are compared
    clean = _stream([synth.logs(93, 300_000).tobytes()])
    for name, b, most in (("bomb", bomb, 16), ("truncated", clean[: len(clean) - 7], 100000)):
        G = impls.Gpu()
        rb = G.Rb(b)
        got = _reads(rb, 65536, most)
        assert rb.r.whole_launches == 0 and rb.r.whole_slot == 0 and not rb.r.whole_decoded, name
        rx = G.Rb(b)
        ez._lib().ez_reader_set_whole(rx.r._h, 0)  # the same handle decoding Read by Read
        assert got == _reads(rx, 65536, most), name
        assert got == _reads(orc.Reader(b=b), 65536, most), name
    assert _reads(impls.Gpu().Rb(clean[: len(clean) - 7]), 65536, 100000)[-1][1] == ez.EUNEXPECTEDEOF
