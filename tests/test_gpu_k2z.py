"""K2z, the batch decoded-size query (ez_decompressed_size_batch: eazy_amd/csrc/ez_decompress_size.hip
and the exact decoder run dry), on hand-built streams, against the oracle.

_run_size runs a batch under max_len hints that give each chunk size and under hint 0, twice each
(the fast kernel with the exact decoder behind it, and the exact decoder alone), and checks per
stream that both report (len(output), error) of the oracle's Reader read to EOF with an ample
buffer; that the result arrays' extra last entry keeps its -7; that the streams handed to the exact
decoder (the workspace's first words: the count, then the stream indices) are exactly the ones the
test states -- the streams the oracle gives an error, plus the forms the fast parse hands over by
design (a MetaReset after output, a wide meta); and that the library reports the chunk size it ran
with (1 for the lane-per-stream kernel that large batches of short streams take).  The input view
lies between two 64-byte guards of 0xFF with in_off[0] != 0; out and out_off are NULL.  All
comparisons are exact equality.  The builders come from tests/k2_streams.py."""

import numpy as np
import pytest

from k2_streams import GUARD, HDR, HDR_1K, META_BREAK, META_RESET, META_VER, _forms, _oracle, assert_valid, cpy, lit, meta, rb

pytestmark = pytest.mark.gpu

HINTS = (4096, 4097, 1 << 20, 0)  # chunk 64, chunk 256, chunk 1024, unknown
LEAD = 5  # bytes of 0xFF inside the input view before in_off[0] and after in_off[count]


def _ample(b):
    return max(1 << 20, 4 * len(b))


def _run_size(cuda, ins, design=(), limit=0, hints=HINTS, expect=None, handed="auto", route=None, ws_init=0, keep=None):
    """expect: {index: (size, status)} instead of the oracle's answer (a stream too large for it);
    design: indices of valid streams the fast parse hands over by design; handed=None: the slow list
    is not checked; route: {hint: what ez_decompressed_size_chunk_last must report} where that is not
    the hint's chunk (1: the lane-per-stream kernel).  ws_init: what the workspace holds when a call
    starts (a fill byte, or a tensor to copy from); it lies between two guards (tests/dirty.py) that
    must be intact afterwards, and the exact decoder alone must leave it as it was.  keep: a list
    that receives the workspace of every run of the fast kernel as it left it.
    Returns the (sizes, statuses) of the first run."""
    import torch

    import eazy_amd as ez
    from dirty import guarded, guards_intact

    count = len(ins)
    coff = LEAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    ff = b"\xff" * (GUARD + LEAD)
    whole = torch.from_numpy(np.frombuffer(ff + b"".join(ins) + ff, np.uint8).copy()).to(cuda)
    comp = whole[GUARD : len(whole) - GUARD]
    assert comp.numel() == int(coff[-1]) + LEAD and coff[0] != 0
    d_coff = torch.from_numpy(coff).to(cuda)
    want = [expect[s] if expect and s in expect else None for s in range(count)]
    for s, b in enumerate(ins):
        if want[s] is None:
            out, err = _oracle(b, _ample(b), limit)
            if err == 2:  # (the oracle's buffer was too small: a golden fuzz input decodes to 14 MB)
                out, err = _oracle(b, 1 << 26, limit)
            assert err != 2, (s, "the oracle's buffer is too small")
            want[s] = (len(out), err)
    bad = {s for s in range(count) if want[s][1] != 0} | set(design)
    first = None
    for hint in hints:
        for exact in (False, True):
            sz = torch.full((count + 1,), -7, dtype=torch.int64, device=cuda)
            st = torch.full((count + 1,), -7, dtype=torch.int32, device=cuda)
            ws_whole, ws = guarded(cuda, ez._lib().ez_decompress_workspace(count), ws_init)
            ws0 = ws.clone()
            ez.decompressed_sizes(comp, d_coff, block_size_limit=limit, sizes=sz, status=st, workspace=ws, exact_only=exact, max_len=hint)
            torch.cuda.synchronize()
            guards_intact(ws_whole, f"hint {hint}, exact {exact}")
            ran = route[hint] if route and hint in route else ez.decompressed_size_chunk(hint)
            assert ez.decompressed_size_chunk_last() == (0 if exact else ran), (hint, exact)
            sz, st = sz.cpu().numpy(), st.cpu().numpy()
            w = ws[: 4 * (count + 1)].cpu().numpy().view(np.uint32)
            assert sz[count] == -7 and st[count] == -7, (hint, exact)
            for s in range(count):
                assert (int(sz[s]), int(st[s])) == want[s], (hint, exact, s, int(sz[s]), int(st[s]), want[s])
            if not exact and handed is not None:
                got = set(int(x) for x in w[1 : 1 + int(w[0])])
                assert int(w[0]) == len(got)
                assert got == bad, (hint, sorted(got), sorted(bad))
            if keep is not None and not exact:
                keep.append(ws.clone())
            if exact:
                assert torch.equal(ws, ws0)  # (the workspace is not used: with the default, its first word stays 0)
            if first is None:
                first = (sz[:count].copy(), st[:count].copy())
            assert np.array_equal(first[0], sz[:count]) and np.array_equal(first[1], st[:count]), (hint, exact)
    return first


# ---------------------------------------------------------------- the streams


def _small_cpy(d, n):
    """cpy(d, n) for n < 124 and d < 252, without a library call (the filler below writes thousands)."""
    return bytes([0x80 | n, d - n]) if d >= n else bytes([0x80 | n, 0xFF, d])


def fill_to(c, target, rng):
    """c plus short literals and copies up to exactly target bytes (tools/k2_size_check.hip's filler)."""
    parts = [c]
    n = len(c)
    while n < target:
        left = target - n
        if left == 1:
            t = b"\x00"  # (one byte: padding)
        elif left <= 100:
            t = bytes([left - 1]) + rb(rng, left - 1)
        elif rng.integers(3) == 0:
            t = _small_cpy(1 + int(rng.integers(200)), 4 + int(rng.integers(60)))
        else:
            k = 1 + int(rng.integers(60))
            t = bytes([k]) + rb(rng, k)
        parts.append(t)
        n += len(t)
    out = b"".join(parts)
    assert len(out) == target
    return out


def _tail3():
    return lit(b"tail!") + cpy(3, 9) + lit(b"zz")


def test_filler_tokens_are_the_encoders():
    assert _small_cpy(30, 20) == cpy(30, 20) and _small_cpy(3, 9) == cpy(3, 9) and _small_cpy(200, 63) == cpy(200, 63)
    assert bytes([5]) + b"abcde" == lit(b"abcde")


_CACHE = {}


def _small_streams():
    """1,025 streams of 40 to 300 bytes."""
    if "small" not in _CACHE:
        rng = np.random.default_rng(211)
        _CACHE["small"] = [fill_to(HDR, 40 + int(rng.integers(261)), rng) for _ in range(1025)]
    return _CACHE["small"]


def _seam_streams(C):
    """Every form with its first byte at each of the last 8 positions before a chunk seam (chunk 3 | 4)
    and before a super-block seam; the super-block starts at 0, or where a 70,000-byte literal ends."""
    if ("seam", C) not in _CACHE:
        rng = np.random.default_rng(223 + C)
        out = []
        # (the streams of one seam share their tokens up to 300 bytes before it: the filler is the slow part)
        far_lit = lit(rb(rng, 70000))
        lead = {}
        for far in (False, True):
            c = HDR + (far_lit if far else b"")
            base = len(c) if far else 0
            for seam in (4 * C, 64 * C):
                lead[(far, seam)] = (fill_to(c, max(len(c), base + seam - 300), rng), base + seam)
        for name, form, _, far in _forms(rng):
            for seam in (4 * C, 64 * C):
                for d in range(1, 9):
                    c, at = lead[(far, seam)]
                    out.append((f"{name}-{seam}-{d}", fill_to(c, at - d, rng) + form + _tail3()))
        _CACHE[("seam", C)] = out
    return _CACHE[("seam", C)]


# ---------------------------------------------------------------- tests


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1025])
def test_counts(cuda, count):
    _run_size(cuda, _small_streams()[:count])


def test_empty_and_header_only(cuda):
    small = _small_streams()[0]
    for ins in ([b""], [HDR], [b"", HDR, b"", small, HDR, b""]):
        sz, st = _run_size(cuda, ins)
        for s, b in enumerate(ins):
            if b in (b"", HDR):
                assert (sz[s], st[s]) == (0, 0)


@pytest.mark.parametrize("C", [64, 256, 1024])
def test_seams(cuda, C):
    named = _seam_streams(C)
    assert len(named) == 21 * 2 * 8
    assert_valid(named)
    _run_size(cuda, [b for _, b in named])


@pytest.mark.parametrize("C", [64, 256, 1024])
def test_super_block_lengths(cuda, C):
    """One stream of 64 x C + 40 input bytes and one of 2 x 64 x C exactly."""
    rng = np.random.default_rng(227 + C)
    ins = [fill_to(HDR, 64 * C + 40, rng), fill_to(HDR, 2 * 64 * C, rng)]
    assert [len(b) for b in ins] == [64 * C + 40, 128 * C]
    sz, st = _run_size(cuda, ins)
    assert list(st) == [0, 0]


def test_literal_skip(cuda):
    """A 70,000-byte literal, then 3 tokens: the body is never staged or read."""
    rng = np.random.default_rng(229)
    sz, st = _run_size(cuda, [HDR + lit(rb(rng, 70000)) + _tail3()])
    assert (sz[0], st[0]) == (70000 + 5 + 9 + 2, 0)


def test_errors(cuda):
    """One stream per status, between two valid ones; size = the bytes produced before the error."""
    import eazy_amd as ez

    rng = np.random.default_rng(233)
    ok = _small_streams()[1]
    body = rb(rng, 2000)
    cases = [
        ("missed meta", b"\x80\x02eazy" + lit(b"ab"), (0, ez.EMISSEDMETA)),
        ("truncated literal", HDR + b"\x03ab", (2, ez.EUNEXPECTEDEOF)),
        ("distance past the window", HDR_1K + lit(body) + cpy(1500, 20) + lit(b"q"), (2000, ez.EOVERFLOW)),
        ("bad magic", b"\x80\x02eazx" + HDR[6:] + lit(b"ab"), (0, ez.EBADMAGIC)),
        ("unsupported version", HDR + lit(b"abc") + meta(META_VER, b"\x01") + lit(b"d"), (3, ez.EUNSUPVER)),
        ("unsupported meta", HDR + lit(b"abcd") + meta(4 << 3) + lit(b"e"), (4, ez.EUNSUPMETA)),
    ]
    ins = [ok]
    for _, b, _ in cases:
        ins += [b, ok]
    sz, st = _run_size(cuda, ins)
    for k, (name, _, want) in enumerate(cases):
        assert (sz[1 + 2 * k], st[1 + 2 * k]) == want, name
    # a length over BlockSizeLimit, with the limit set (the window, 1 KiB, is within it)
    ins = [ok, HDR_1K + lit(b"abc") + lit(body) + lit(b"q"), HDR_1K + lit(body[:1024]) + cpy(5, 1024)]
    sz, st = _run_size(cuda, ins, limit=1024)
    assert (sz[1], st[1]) == (3, ez.EBLOCKLIMIT)
    assert (sz[2], st[2]) == (2048, 0)


def test_valid_only_for_the_exact_path(cuda):
    """Streams the Reader accepts and the fast parse hands over by design."""
    ok = _small_streams()[2]
    reset_late = HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b")
    wide = HDR + lit(b"abc") + b"\x80" + bytes([META_BREAK | 6, 0]) + lit(b"de")
    sz, st = _run_size(cuda, [ok, reset_late, ok, wide], design=(1, 3))
    assert (sz[1], st[1]) == (2, 0)
    assert (sz[3], st[3]) == (5, 0)


def test_bomb(cuda):
    """41 bytes that claim over 10 GiB: reported in 64 bits, by arithmetic on the headers alone (the dry
    decoder never loops over output bytes).  The expected size is the test's own sum; the oracle is not run."""
    bomb = HDR + lit(b"x") + cpy(1, 1 << 29) * 20
    assert len(bomb) < 200
    want = 1 + 20 * (1 << 29)
    assert want > 10 << 30
    ok = _small_streams()[3]
    sz, st = _run_size(cuda, [ok, bomb, ok], expect={1: (want, 0)})
    assert (int(sz[1]), int(st[1])) == (want, 0)


def test_lane_per_stream(cuda):
    """4,096 streams or more under a hint of at most 4 KiB take the lane-per-stream kernel (reported as
    chunk 1), one stream fewer the wave kernel: the same answers, errors and hand-overs included."""
    import eazy_amd as ez

    rng = np.random.default_rng(241)
    small = _small_streams()
    special = {7: b"", 64: HDR, 100: HDR + b"\x03ab", 1000: HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b"),
               2047: fill_to(HDR, 4096, rng), 4095: HDR + lit(rb(rng, 3000)) + _tail3(), 4096: b"\x80\x02eazy" + lit(b"ab")}
    ins = [special.get(s, small[s % len(small)]) for s in range(4097)]
    for count, ran in ((4097, 1), (4096, 1), (4095, 64)):
        sz, st = _run_size(cuda, ins[:count], design=(1000,), hints=(4096, 0), route={4096: ran})
        assert (sz[100], st[100]) == (2, ez.EUNEXPECTEDEOF) and (sz[1000], st[1000]) == (2, 0)


def test_hint_independence(cuda):
    rng = np.random.default_rng(239)
    small = _small_streams()
    ins = small[:20] + [b"", HDR, HDR + b"\x03ab", fill_to(HDR, 64 * 256 + 40, rng), HDR + lit(rb(rng, 70000)) + _tail3(),
                        HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b"), fill_to(HDR, 5000, rng)] + small[20:40]
    _run_size(cuda, ins, design=(25,), hints=(0, 1, 4096, 4097, 512 << 10, (512 << 10) + 1, 1 << 31))


@pytest.mark.parametrize("count,size", [(256, 4096), (8, 256 << 10)])
def test_round_trip(cuda, count, size):
    """Synthetic logs through compress_batch, then decoded without knowing their lengths."""
    import torch

    import eazy_amd as ez
    from eazy_amd import synth

    host = synth.logs(11, count * size)
    offs = synth.batch_offsets(count, size)
    data = torch.from_numpy(host).to(cuda)
    cb = ez.compress_batch(data, torch.from_numpy(offs).to(cuda), ez.MiB, 1024, max_len=size)
    packed, poff = ez.pack(cb)
    out, out_off, sizes, status = ez.decompress_batch_sized(packed, poff)
    torch.cuda.synchronize()
    assert int(cb.status.abs().sum()) == 0
    assert status.cpu().numpy().tolist() == [0] * count
    assert sizes.cpu().numpy().tolist() == [size] * count
    oo = out_off.cpu().numpy()
    o = out.cpu().numpy()
    assert all(int(x) % 16 == 0 for x in oo)
    for s in range(count):
        assert o[oo[s] : oo[s] + size].tobytes() == host[offs[s] : offs[s + 1]].tobytes(), s
    # slots of exactly the reported sizes, no rounding
    need, st0 = ez.decompressed_sizes(packed, poff, max_len=int((poff[1:] - poff[:-1]).max().item()))
    exact_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cuda), torch.cumsum(need, 0)])
    out2, sizes2, status2 = ez.decompress_batch(packed, poff, exact_off)
    torch.cuda.synchronize()
    assert st0.cpu().numpy().tolist() == [0] * count and need.cpu().numpy().tolist() == [size] * count
    assert status2.cpu().numpy().tolist() == [0] * count and sizes2.cpu().numpy().tolist() == [size] * count
    assert out2[: count * size].cpu().numpy().tobytes() == host.tobytes()


def test_golden_corpora(cuda):
    """Sizes and statuses on the golden corpora equal the oracle's (no claim about the slow list)."""
    from golden_data import h, load

    g = load()
    ins = [h(e["input"]) for e in g["fuzz_reader"]]
    for e in g["fuzz_writer"]:
        ins += [h(v) for k, v in sorted(e.items()) if k.startswith(("single_", "stream_")) and isinstance(v, str)]
    ins += [h(v) for k, v in sorted(g["multi_write"].items()) if k.startswith("stream_") and isinstance(v, str)]
    for e in g["synthetic_logs"]:
        ins += [h(v) for k, v in sorted(e.items()) if k.startswith("stream_")]
    assert len(ins) >= 20 + 9 * 3
    _run_size(cuda, ins, handed=None)
