"""K2g's parts route on the GPU (ez_decompress_segs_parts.hip): the segment query of long concatenated
streams cut over many waves, forced with ez_select_segments_route('p') and given b->in_bytes.

The query runs on the hand-built streams of the host check (tools/k2_segs_parts_check.hip, which writes
them and the cuts of its single-lane walk with --dump) at both chunk sizes, on a sub-batch view
(in_off[0] and out_off[0] are not 0), into 0xA5-guarded arrays, after the library's cached scratch was
filled with 0xA5: its arrays equal the host walk's and the wave route's ('v').  The route's counters,
the in_bytes hint (under-stated by 1, unknown, over-stated three times), the segmented decode and the
size query over oracle-written streams of 20 segments follow.  All comparisons are exact equality."""

import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import eazy_amd as ez
import oracle as orc
from test_k2_segs_parts import build_check

pytestmark = pytest.mark.gpu

PAD, LEAD = 37, 5  # bytes before in_off[0] and out_off[0]: a sub-batch view
RESET = b"\x80\x10\x14"
A5 = int(np.frombuffer(b"\xa5" * 8, np.int64)[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """[(name, BlockSizeLimit, stream, [(input position, output before)])] from the host check."""
    tmp = tmp_path_factory.mktemp("k2_segs_parts_gpu")
    f = tmp / "streams.bin"
    p = subprocess.run([build_check(tmp), "--dump", str(f)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    raw, at, res = f.read_bytes(), 0, []
    while at < len(raw):
        nname, limit, nb, ncut, _stop = struct.unpack_from("<5Q", raw, at)
        at += 40
        name = raw[at : at + nname].decode()
        at += nname
        b = raw[at : at + nb]
        at += nb
        cuts = [struct.unpack_from("<2Q", raw, at + 16 * k) for k in range(ncut)]
        at += 16 * ncut
        res.append((name, limit, b, cuts))
    assert len(res) > 60 and sum(len(c) for _, _, _, c in res) > 10000
    return res


def _inputs(cuda, ins, caps):
    import torch

    coff = PAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    ooff = LEAD + np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"\xff" * PAD + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
    return comp[: len(comp) - 16], torch.from_numpy(coff).to(cuda), torch.from_numpy(ooff).to(cuda), coff, ooff


def _query(cuda, comp, d_coff, d_ooff, count, cap, limit, max_len, in_bytes, route):
    """ez_stream_segments_batch under a route, on 0xA5 scratch, into guarded arrays -> ((seg_idx, seg_in,
    seg_out, seg_total) as numpy, the route's counters); the guards and the entries past the written ones
    are checked."""
    import torch
    from dirty import guarded, guards_intact

    L = ez._lib()
    arrs = []
    for n in (count + 1, cap + 1, cap + 1, 2):
        whole = torch.full(((n + 16) * 8,), 0xA5, dtype=torch.uint8, device=cuda).view(torch.int64)
        arrs.append((whole, whole[8 : 8 + n]))
    ws_whole, ws = guarded(cuda, L.ez_segments_workspace(count), 0xA5)
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, d_ooff.data_ptr(), None, None, count, max_len, in_bytes, 0)
    ez.select_segments_route(route)
    try:
        ez.fill_cached(0xA5)
        st = L.ez_stream_segments_batch(limit, C.byref(b), arrs[0][1].data_ptr(), arrs[1][1].data_ptr(), arrs[2][1].data_ptr(), cap,
                                        arrs[3][1].data_ptr(), ws.data_ptr(), ez._stream_ptr(None))
        assert st == ez.OK, st
        torch.cuda.synchronize()
        last = ez.segments_parts_last()
    finally:
        ez.select_segments_route("")
    out = []
    for whole, view in arrs:
        w = whole.cpu().numpy()
        assert (w[:8] == A5).all() and (w[-8:] == A5).all()
        out.append(view.cpu().numpy())
    guards_intact(ws_whole, "the segment query")
    written = int(out[3][0])
    assert (out[1][written + 1 :] == A5).all() and (out[2][written + 1 :] == A5).all()
    return out, last


def _expected(group, coff, ooff):
    idx, sin, sout = [0], [], []
    for s, (_, _, _, cuts) in enumerate(group):
        sin.append(coff[s])
        sout.append(ooff[s])
        for pos, o in cuts:
            sin.append(coff[s] + pos)
            sout.append(min(ooff[s] + o, ooff[s + 1]))
        idx.append(idx[-1] + len(cuts) + 1)
    return np.array(idx), np.array(sin + [coff[-1]]), np.array(sout + [ooff[-1]])


def _caps(group):
    """slots: room for everything; every fifth stream with cuts ends inside its output (clamped cuts); one slot of 0"""
    caps = []
    for s, (_, _, _, cuts) in enumerate(group):
        last = cuts[-1][1] if cuts else 0
        caps.append(0 if s == 7 else (cuts[len(cuts) // 2][1] - 1 if cuts and s % 5 == 3 else last + 1 + s % 9))
    return caps


def _groups(dumped):
    """per BlockSizeLimit: the dumped streams with an empty and a 10-byte stream among them"""
    for limit in sorted(set(e[1] for e in dumped)):
        group = [e for e in dumped if e[1] == limit]
        group.insert(2, ("empty", limit, b"", []))
        group.insert(5, ("ten bytes", limit, b"\x80\x02eazy\x80\x10\x14\x00", []))
        yield limit, group


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:4])


@pytest.mark.parametrize("max_len", [0, 1 << 20])
def test_query_equals_host_walk_and_wave_route(cuda, dumped, max_len):
    chunk = {0: 256, 1 << 20: 1024}[max_len]
    assert ez._lib().ez_decompressed_size_chunk(max_len) == chunk
    P = 64 * chunk
    for limit, group in _groups(dumped):
        caps = _caps(group)
        comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, [e[2] for e in group], caps)
        idx, sin, sout = _expected(group, coff, ooff)
        found, count = int(idx[-1]), len(group)
        in_bytes = int(coff[-1] - coff[0])
        got, last = _query(cuda, comp, d_coff, d_ooff, count, found + 3, limit, max_len, in_bytes, "p")
        seg_idx, seg_in, seg_out, total = got
        assert tuple(total) == (found, found)
        bad = np.flatnonzero(seg_idx != idx)
        assert bad.size == 0, (group[int(bad[0]) - 1][0], seg_idx[bad[:4]], idx[bad[:4]])
        for g, want in ((seg_in[: found + 1], sin), (seg_out[: found + 1], sout)):
            bad = np.flatnonzero(g != want)
            assert bad.size == 0, (group[int(np.searchsorted(idx, bad[0], "right")) - 1][0], g[bad[:4]], want[bad[:4]])
        wave, wlast = _query(cuda, comp, d_coff, d_ooff, count, found + 3, limit, max_len, in_bytes, "v")
        _same(got, wave, "parts against the wave route")
        assert wlast == (0, 0, 0, 0)
        # the counters: every part in the first pass; records taken and parts walked again; the parts that hold a cut filled
        parts = sum(-(-len(e[2]) // P) for e in group)
        filled = len(set((s, pos // P) for s, e in enumerate(group) for pos, _ in e[3]))
        assert last[0] == parts and last[1] > 0 and last[2] > 0 and last[3] == filled, (last, parts, filled)
        # the hint: under-stated by 1 (the wave route walks the batch: counters 0), unknown, over-stated three times
        for hint, ran in ((in_bytes - 1, False), (0, False), (3 * in_bytes, True)):
            again, hlast = _query(cuda, comp, d_coff, d_ooff, count, found + 3, limit, max_len, hint, "p")
            _same(got, again, f"in_bytes {hint}")
            assert hlast == (last if ran else (0, 0, 0, 0)), (hint, hlast)
        # seg_cap one short of the segments found: one segment per stream, seg_total = (count, found)
        if found > count:
            (seg_idx, seg_in, seg_out, total), _ = _query(cuda, comp, d_coff, d_ooff, count, found - 1, limit, max_len, in_bytes, "p")
            assert tuple(total) == (count, found) and list(seg_idx) == list(range(count + 1))
            assert list(seg_in[: count + 1]) == list(coff) and list(seg_out[: count + 1]) == list(ooff)


@pytest.mark.parametrize("count", [1025, 2049])
def test_layout_of_several_streams_per_thread(cuda, count):
    """count > 1,024: kp_layout's threads take 2 and 3 streams each and the threads past the end none.
    test_gpu_k2z_parts.many_streams (tiny streams of one part, every 97th of two parts, every 101st
    empty; none holds a cut), forced, chunk 256, in_bytes exact: the arrays of the wave route, a segment
    per stream, every part in the first pass; in_bytes one short: the same arrays, no part walked."""
    from test_gpu_k2z_parts import many_streams

    ins, _ = many_streams(count)
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, [4 * len(b) + 16 for b in ins])
    in_bytes = int(coff[-1] - coff[0])
    wave, wlast = _query(cuda, comp, d_coff, d_ooff, count, count + 3, 0, 0, in_bytes, "v")
    assert tuple(wave[3]) == (count, count) and wlast == (0, 0, 0, 0)
    got, last = _query(cuda, comp, d_coff, d_ooff, count, count + 3, 0, 0, in_bytes, "p")
    _same(got, wave, "parts against the wave route")
    assert last[0] == sum(-(-len(b) // (64 * 256)) for b in ins) and last[1] + last[2] <= last[0], last
    again, hlast = _query(cuda, comp, d_coff, d_ooff, count, count + 3, 0, 0, in_bytes - 1, "p")
    _same(again, wave, "in_bytes one short")
    assert hlast == (0, 0, 0, 0), hlast


def _log_lines(rng, n):
    out = bytearray()
    while len(out) < n:
        out += b"2026-01-01T00:00:%02d INFO tenant-%d GET /api/v1/items/%d status=200 bytes=%d\n" % (
            rng.integers(60), rng.integers(13), rng.integers(5000), rng.integers(100000))
    return bytes(out[:n])


@pytest.fixture(scope="module")
def reset_streams():
    """8 streams of 20 Writes of 16 KiB with Writer.Reset between them, by the oracle's Writer."""
    rng = np.random.default_rng(17)
    ins, plain = [], []
    for s in range(8):
        w = orc.Writer(1 << 20, 1024)
        comp, text = b"", b""
        for g in range(20):
            if g:
                w.reset()
            p = _log_lines(rng, 16384 - 13 * s + g)
            assert w.write(p) == (len(p), 0)
            comp += w.sink
            w.sink_clear()
            text += p
        ins.append(comp)
        plain.append(text)
        assert orc.decompress(comp)[:2] == (text, 0)
    return ins, plain


def test_segmented_decode_under_parts_route(cuda, reset_streams):
    import torch

    ins, plain = reset_streams
    caps = [len(p) for p in plain]
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, caps)
    res = []
    for exact in (False, True):
        out = torch.full((int(ooff[-1]) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        sz = torch.full((8,), -7, dtype=torch.int64, device=cuda)
        st = torch.full((8,), -7, dtype=torch.int32, device=cuda)
        if exact:
            ez.decompress_batch(comp, d_coff, d_ooff, out=out, sizes=sz, status=st, exact_only=True)
        else:
            ez.select_segments_route("p")
            try:
                ez.fill_cached(0xA5)
                ez.decompress_batch_segmented(comp, d_coff, d_ooff, out=out, sizes=sz, status=st)
                torch.cuda.synchronize()
                segs = ez.segments_last()
            finally:
                ez.select_segments_route("")
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), sz.cpu().numpy(), st.cpu().numpy()))
    (out, sz, st), (xout, xsz, xst) = res
    assert segs[:2] == (160, 0)
    assert np.array_equal(sz, xsz) and np.array_equal(st, xst) and (st == 0).all() and list(sz) == caps
    assert np.array_equal(out, xout)
    assert out[LEAD : int(ooff[-1])].tobytes() == b"".join(plain)
    assert (out[:LEAD] == 0xA5).all() and (out[int(ooff[-1]) :] == 0xA5).all()


def test_sizes_under_parts_route(cuda, reset_streams, dumped):
    import torch

    ins, plain = reset_streams
    for batch, clean in ((ins, True), ([e[2] for e in dumped if e[1] == 0], False)):
        n = len(batch)
        comp, d_coff, _, coff, _ = _inputs(cuda, batch, [0] * n)
        want, wst = ez.decompressed_sizes(comp, d_coff, exact_only=True)
        ws = torch.full((ez._lib().ez_decompress_workspace(n),), 0xA5, dtype=torch.uint8, device=cuda)
        ez.select_segments_route("p")
        try:
            ez.fill_cached(0xA5)
            got, gst = ez.decompressed_sizes(comp, d_coff, workspace=ws, in_bytes=int(coff[-1] - coff[0]))
            torch.cuda.synchronize()
            counts = ez.decompressed_size_segs_last(ws, n)
            stage = ez.segments_parts_last()
            if clean:
                out, out_off, sz, st = ez.decompress_batch_sized(comp, d_coff)
                torch.cuda.synchronize()
        finally:
            ez.select_segments_route("")
        assert torch.equal(got, want) and torch.equal(gst, wst)
        assert counts[0] == counts[1] + counts[2]
        if clean:
            assert counts == (n, n, 0)
            # the stage took the route: every part of the handed-over streams in its first pass, nothing filled
            assert stage[0] == sum(-(-len(b) // (64 * 256)) for b in batch) and stage[1] + stage[2] > 0 and stage[3] == 0, stage
            assert (st == 0).all() and sz.cpu().tolist() == [len(p) for p in plain]
            o, off = out.cpu().numpy(), out_off.cpu().numpy()
            for s, p in enumerate(plain):
                assert o[off[s] : off[s] + len(p)].tobytes() == p, s


def test_route_entry_points(cuda):
    L = ez._lib()
    assert L.ez_select_segments_route(ord("x")) == ez.EINVAL
    assert L.ez_select_segments_route(ord("p")) == 0 and L.ez_select_segments_route(ord("v")) == 0 and L.ez_select_segments_route(0) == 0
    assert L.ez_segments_parts_last(None) == ez.EINVAL
    c = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.ez_segments_parts_last(c) == 0
