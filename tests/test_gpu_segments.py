"""K2g on the GPU: the segment query (ez_stream_segments_batch) and the decode over its cuts
(ez_decompress_batch_segmented), for streams that hold MetaResets after output.

The query runs on the hand-built streams of the host check (tools/k2_segs_check.hip, which writes them
and the cuts of its single-lane walk with --dump) at the three chunk sizes; its arrays equal the host
walk's, inside 0xA5 sentinels, on a sub-batch view (in_off[0] and out_off[0] are not 0).  The
segmented decode equals decompress_batch(exact_only=True) on the same batch: sizes, statuses and the
bytes of every stream, with the OK streams' bytes the oracle's, for the library's usual odd slots,
exact slots and slots that end at, before and after every segment boundary.  A batch of 64 streams of
4 segments written by the oracle's Writer with Reset between its Writes goes to the exact decoder
whole with decompress_batch, and to the fast decoders segment by segment here.  All comparisons are
exact equality."""

import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import eazy_amd as ez
import oracle as orc
from k2_streams import HDR, _forms, _need, _oracle, _slot, cpy, lit, rb
from test_k2_segments import build_check

pytestmark = pytest.mark.gpu

PAD, LEAD = 37, 5  # bytes before in_off[0] and out_off[0]: a sub-batch view
RESET = b"\x80\x10\x14"


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """[(name, BlockSizeLimit, stream, [(input position, output before)])] from the host check."""
    tmp = tmp_path_factory.mktemp("k2_segs_gpu")
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
    assert len(res) > 300 and sum(len(c) for _, _, _, c in res) > 500
    return res


def _guarded(cuda, n, dtype):
    """A tensor of n elements between two guards of 8 elements, everything 0xA5 bytes."""
    import torch

    whole = torch.full(((n + 16) * dtype.itemsize,), 0xA5, dtype=torch.uint8, device=cuda).view(dtype)
    return whole, whole[8 : 8 + n]


def _sentinel(dtype):
    return int(np.frombuffer(b"\xa5" * 8, np.int64)[0]) if dtype.itemsize == 8 else int(np.frombuffer(b"\xa5" * 4, np.int32)[0])


def _inputs(cuda, ins, caps):
    import torch

    coff = PAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    ooff = LEAD + np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"\xff" * PAD + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
    return comp[: len(comp) - 16], torch.from_numpy(coff).to(cuda), torch.from_numpy(ooff).to(cuda), coff, ooff


def _query(cuda, comp, d_coff, d_ooff, count, cap, limit=0, max_len=0, ws_init=0xA5, keep=None):
    """ez_stream_segments_batch into guarded arrays -> (seg_idx, seg_in, seg_out, seg_total) as numpy,
    seg_in / seg_out whole (cap + 1 entries); the guards and the entries past the written ones are checked.
    ws_init: what the workspace holds when the call starts (a fill byte, or a tensor to copy from), between
    its two guards (tests/dirty.py); keep: a list that receives the workspace as the query left it."""
    import torch
    from dirty import guarded, guards_intact

    L = ez._lib()
    arrs = [_guarded(cuda, n, torch.int64) for n in (count + 1, cap + 1, cap + 1, 2)]
    ws_whole, ws = guarded(cuda, L.ez_segments_workspace(count), ws_init)
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, d_ooff.data_ptr(), None, None, count, max_len, 0, 0)
    st = L.ez_stream_segments_batch(limit, C.byref(b), arrs[0][1].data_ptr(), arrs[1][1].data_ptr(), arrs[2][1].data_ptr(), cap,
                                    arrs[3][1].data_ptr(), ws.data_ptr(), ez._stream_ptr(None))
    assert st == ez.OK, st
    torch.cuda.synchronize()
    a5 = _sentinel(np.dtype(np.int64))
    out = []
    for whole, view in arrs:
        w = whole.cpu().numpy()
        assert (w[:8] == a5).all() and (w[-8:] == a5).all()
        out.append(view.cpu().numpy())
    guards_intact(ws_whole, "the segment query")
    if keep is not None:
        keep.append(ws.clone())
    written = int(out[3][0])
    assert (out[1][written + 1 :] == a5).all() and (out[2][written + 1 :] == a5).all()
    return out


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


@pytest.mark.parametrize("max_len", [4096, 1 << 16, 1 << 20, 0])
def test_query_equals_host_walk(cuda, dumped, max_len):
    assert ez._lib().ez_decompressed_size_chunk(max_len) == {4096: 64, 1 << 16: 256, 1 << 20: 1024, 0: 256}[max_len]
    for limit in sorted(set(e[1] for e in dumped)):
        group = [e for e in dumped if e[1] == limit]
        # slots: room for everything; every fifth stream with cuts ends inside its output (clamped cuts), one slot of 0
        caps = []
        for s, (_, _, b, cuts) in enumerate(group):
            last = cuts[-1][1] if cuts else 0
            caps.append(0 if s == 7 else (cuts[len(cuts) // 2][1] - 1 if cuts and s % 5 == 3 else last + 1 + s % 9))
        comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, [e[2] for e in group], caps)
        idx, sin, sout = _expected(group, coff, ooff)
        found = int(idx[-1])
        seg_idx, seg_in, seg_out, total = _query(cuda, comp, d_coff, d_ooff, len(group), found + 3, limit, max_len)
        assert tuple(total) == (found, found)
        bad = np.flatnonzero(seg_idx != idx)
        assert bad.size == 0, (group[int(bad[0]) - 1][0], seg_idx[bad[:4]], idx[bad[:4]])
        for got, want in ((seg_in[: found + 1], sin), (seg_out[: found + 1], sout)):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (group[int(np.searchsorted(idx, bad[0], "right")) - 1][0], got[bad[:4]], want[bad[:4]])


def test_query_edges(cuda, dumped):
    import torch

    L = ez._lib()
    # count == 0: the arrays' first entries and seg_total
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, [], [])
    seg_idx, seg_in, seg_out, total = _query(cuda, comp, d_coff, d_ooff, 0, 0)
    assert (seg_idx[0], seg_in[0], seg_out[0], tuple(total)) == (0, PAD, LEAD, (0, 0))
    # an empty stream among others: one segment
    four = next(e for e in dumped if e[0].startswith("C256 packed resets x3"))
    ins, cuts = [b"", four[2], b"", HDR], four[3]
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, [0, 100, 3, 0])
    seg_idx, seg_in, seg_out, total = _query(cuda, comp, d_coff, d_ooff, 4, 10)
    assert tuple(total) == (7, 7) and list(seg_idx) == [0, 1, 5, 6, 7]
    assert list(seg_in[:8]) == [coff[0], coff[1]] + [coff[1] + p for p, _ in cuts] + [coff[2], coff[3], coff[4]]
    # seg_cap == count with more found: one segment per stream, seg_total = (count, found)
    seg_idx, seg_in, seg_out, total = _query(cuda, comp, d_coff, d_ooff, 4, 4)
    assert tuple(total) == (4, 7) and list(seg_idx) == [0, 1, 2, 3, 4]
    assert list(seg_in) == list(coff) and list(seg_out) == list(ooff)
    # seg_cap < count and NULL arrays are refused, nothing is launched
    arr = torch.zeros(16, dtype=torch.int64, device=cuda)
    ws = torch.zeros(L.ez_segments_workspace(4), dtype=torch.uint8, device=cuda)
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, d_ooff.data_ptr(), None, None, 4, 0, 0, 0)
    p = arr.data_ptr()
    assert L.ez_stream_segments_batch(0, C.byref(b), p, p, p, 3, p, ws.data_ptr(), None) == ez.EINVAL
    for k in range(5):
        a = [p, p, p, 8, p, ws.data_ptr()]
        a[k if k < 3 else k + 1] = None
        assert L.ez_stream_segments_batch(0, C.byref(b), *a, None) == ez.EINVAL
    nb = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, None, None, 4, 0, 0, 0)
    assert L.ez_stream_segments_batch(0, C.byref(nb), p, p, p, 8, p, ws.data_ptr(), None) == ez.EINVAL
    with pytest.raises(ez.Panic):
        ez.stream_segments(comp, d_coff, d_ooff, seg_cap=3)
    # the Python mirror: too little room asks again
    seg_idx, seg_in, seg_out, total = ez.stream_segments(comp, d_coff, d_ooff)
    assert tuple(total.cpu().numpy()) == (7, 7) and seg_in.numel() == 8 and seg_out.numel() == 8
    torch.cuda.synchronize()
    assert int(arr.sum()) == 0


def _decode_both(cuda, ins, caps, limit=0, scratch=None):
    """The segmented decode and the exact decoder on one batch: equal sizes, statuses and bytes,
    sentinels intact outside every slot and in the slack of the streams that end OK, the OK streams'
    bytes the oracle's.  scratch: the segmented decode's workspace is the library's own, so the
    counterpart of the other runners' ws_init is a fill byte for ez.fill_cached, applied right before
    the segmented decode (None: the scratch as the calls before left it).
    Returns (sizes, statuses, the first decoder of the segmented decode)."""
    import torch

    count = len(ins)
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, caps)
    host_in = comp.cpu().numpy().copy()
    res = []
    for exact in (False, True):
        out = torch.full((int(ooff[-1]) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        sz = torch.full((count,), -7, dtype=torch.int64, device=cuda)
        st = torch.full((count,), -7, dtype=torch.int32, device=cuda)
        if exact:
            ez.decompress_batch(comp, d_coff, d_ooff, block_size_limit=limit, out=out, sizes=sz, status=st, exact_only=True)
        else:
            if scratch is not None:
                ez.fill_cached(scratch)
            ez.decompress_batch_segmented(comp, d_coff, d_ooff, block_size_limit=limit, out=out, sizes=sz, status=st)
            took = ez.decompress_kernel_last()
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), sz.cpu().numpy(), st.cpu().numpy()))
    (out, sz, st), (xout, xsz, xst) = res
    bad = np.flatnonzero((sz != xsz) | (st != xst))
    assert bad.size == 0, (bad[:4], sz[bad[:4]], xsz[bad[:4]], st[bad[:4]], xst[bad[:4]], [caps[int(k)] for k in bad[:4]])
    inside = np.zeros(len(out), bool)
    for s, b in enumerate(ins):
        o, n = int(ooff[s]), int(sz[s])
        assert 0 <= n <= caps[s]
        assert out[o : o + n].tobytes() == xout[o : o + n].tobytes(), s
        inside[o : o + (n if st[s] == 0 else caps[s])] = True
        want, err = _oracle(b, caps[s], limit)
        if err == 2:
            assert st[s] == ez.ENOSPC, (s, st[s])
            continue
        assert (st[s], n) == (err, len(want)), (s, st[s], err, n, len(want))
        if err == 0:
            assert out[o : o + n].tobytes() == want, s
    for name, a in (("segmented", out), ("exact", xout)):
        stray = np.flatnonzero(~inside & (a != 0xA5))
        assert stray.size == 0, (name, stray[:8])
    assert np.array_equal(comp.cpu().numpy(), host_in), "the input was written"
    return sz, st, took


def _short(dumped, limit):
    return [e for e in dumped if e[1] == limit and len(e[2]) < 60000]


@pytest.mark.parametrize("slots", ["odd", "exact"])
def test_decode_equals_exact_decoder(cuda, dumped, slots):
    for limit in sorted(set(e[1] for e in dumped)):
        group = _short(dumped, limit) + [e for e in dumped if e[1] == limit and len(e[2]) >= 60000][:6]
        ins = [e[2] for e in group]
        need = [_need(b, limit) for b in ins]
        caps = [_slot(s, n) if slots == "odd" else n for s, n in enumerate(need)]
        _, st, _ = _decode_both(cuda, ins, caps, limit)
        assert (st != 0).sum() > 0 and (limit != 0 or (st == 0).sum() > len(ins) // 2)
        segs = ez.segments_last()
        assert segs[0] == len(group) + sum(len(e[3]) for e in group) and segs[2] <= 1


def test_decode_slots_at_every_segment_boundary(cuda, dumped):
    """A 4-segment stream in slots that end 1 before, at and 1 after every segment boundary, and in a
    slot of 0: the ENOSPC cases, whose size is the exact decoder's."""
    rng = np.random.default_rng(5)
    b, bounds = b"", []
    for g in range(4):
        b += (HDR if g == 0 else RESET) + lit(rb(rng, 300 + 50 * g)) + cpy(100, 700) + lit(rb(rng, 40)) + cpy(3, 200 + g)
        bounds.append(_need(b))
    caps = [0] + [n + d for n in bounds for d in (-1, 0, 1)] + [bounds[-1] + 40]
    sz, st, _ = _decode_both(cuda, [b] * len(caps), caps)
    want = [ez.OK if c >= bounds[-1] else ez.ENOSPC for c in caps]
    assert list(st) == want and list(sz) == [min(c, bounds[-1]) for c in caps]


def _log_lines(rng, n):
    out = bytearray()
    while len(out) < n:
        out += b"2026-01-01T00:00:%02d INFO tenant-%d GET /api/v1/items/%d status=200 bytes=%d\n" % (
            rng.integers(60), rng.integers(13), rng.integers(5000), rng.integers(100000))
    return bytes(out[:n])


@pytest.fixture(scope="module")
def reset_batch():
    """64 streams of 4 Writes of about 8 KiB with Writer.Reset between them, by the oracle's Writer."""
    rng = np.random.default_rng(11)
    ins, plain = [], []
    for s in range(64):
        w = orc.Writer(1 << 20, 1024)
        comp, text = b"", b""
        for g in range(4):
            if g:
                w.reset()
            p = _log_lines(rng, 8192 - 17 * (s % 5) + g)
            assert w.write(p) == (len(p), 0)
            comp += w.sink
            w.sink_clear()
            text += p
        ins.append(comp)
        plain.append(text)
        assert comp.count(RESET) >= 4 and orc.decompress(comp)[:2] == (text, 0)
    return ins, plain


def test_reset_streams_leave_the_exact_decoder(cuda, reset_batch):
    import torch

    ins, plain = reset_batch
    caps = [len(p) for p in plain]
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, caps)
    # today's call: every stream is handed to the exact decoder (the workspace's first word counts them)
    ws = torch.zeros(ez._lib().ez_decompress_workspace(64), dtype=torch.uint8, device=cuda)
    out, sz, st = ez.decompress_batch(comp, d_coff, d_ooff, workspace=ws)
    torch.cuda.synchronize()
    assert int(ws[:4].cpu().numpy().view(np.uint32)[0]) == 64 and (st == 0).all()
    # segment by segment: 256 segments, none handed over, no retry
    out = torch.full((int(ooff[-1]) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    out, sz, st = ez.decompress_batch_segmented(comp, d_coff, d_ooff, out=out)
    torch.cuda.synchronize()
    assert ez.segments_last() == (256, 0, 0)
    assert (st == 0).all() and sz.cpu().tolist() == caps
    got = out.cpu().numpy()
    assert got[LEAD : int(ooff[-1])].tobytes() == b"".join(plain)
    assert (got[:LEAD] == 0xA5).all() and (got[int(ooff[-1]) :] == 0xA5).all()
    seg_idx, seg_in, seg_out, total = ez.stream_segments(comp, d_coff, d_ooff, seg_cap=256, max_len=max(len(b) for b in ins))
    assert tuple(total.cpu().numpy()) == (256, 256) and seg_idx.cpu().tolist() == list(range(0, 257, 4))
    ez.release_cached()
    assert ez.segments_last()[:1] == (256,)


def test_batch_without_late_reset(cuda):
    """tests/k2_streams.py forms: one segment per stream, results identical to decompress_batch."""
    import torch

    rng = np.random.default_rng(3)
    ins = [HDR + lit(rb(rng, 900)) + f + lit(rb(rng, 5)) + cpy(3, 9) for _, f, _, big in _forms(rng) if not big] + [b"", HDR]
    caps = [_slot(s, _need(b)) for s, b in enumerate(ins)]
    comp, d_coff, d_ooff, coff, ooff = _inputs(cuda, ins, caps)
    seg_idx, seg_in, seg_out, total = ez.stream_segments(comp, d_coff, d_ooff, seg_cap=len(ins))
    assert tuple(total.cpu().numpy()) == (len(ins), len(ins)) and seg_idx.cpu().tolist() == list(range(len(ins) + 1))
    assert seg_in.cpu().tolist() == list(coff) and seg_out.cpu().tolist() == list(ooff)
    res = []
    for seg in (True, False):
        out = torch.full((int(ooff[-1]) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        f = ez.decompress_batch_segmented if seg else ez.decompress_batch
        out, sz, st = f(comp, d_coff, d_ooff, out=out)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), sz.cpu().numpy(), st.cpu().numpy()))
    for a, b in zip(*res):
        assert (a == b).all()
    segs = ez.segments_last()  # (the slots under 16 bytes are the exact decoder's)
    assert (res[0][2] == 0).all() and (segs[0], segs[2]) == (len(ins), 0)
    _decode_both(cuda, ins, caps)


@pytest.mark.parametrize("kind", ["r", "t", ""])
def test_mixed_batch_under_each_first_decoder(cuda, reset_batch, dumped, kind):
    rng = np.random.default_rng(9)
    valid = reset_batch[0][:5]
    damaged = [e[2] for e in dumped if " in segment 2 of 4" in e[0] and e[1] == 0]
    plain = [HDR + lit(rb(rng, 3000)) + cpy(500, 2000), HDR + lit(rb(rng, 70)), HDR]
    ins = valid[:2] + damaged + plain[:1] + [b""] + valid[2:] + plain[1:] + [b""]
    assert len(damaged) == 3
    caps = [_slot(s, _need(b)) for s, b in enumerate(ins)]
    ez.select_decompress_kernel(kind)
    try:
        _, st, took = _decode_both(cuda, ins, caps)
    finally:
        ez.select_decompress_kernel("")
    assert took == (kind or "r") and sorted(np.flatnonzero(st != 0)) == [2, 3, 4]
    segs = ez.segments_last()
    assert segs[0] == 5 * 4 + 3 * 3 + 3 + 2 and segs[1] >= 3
