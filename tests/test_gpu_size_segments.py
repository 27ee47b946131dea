"""The size query on concatenated streams (a MetaReset after output): K2g's walk behind K2z's kernels
(k2g_size, eazy_amd/csrc/ez_decompress_segs.hip) sizes them on the device, and decompress_batch_sized
then decodes them segment by segment.

The streams are the host check's (tools/k2_segs_check.hip --dump), grouped by BlockSizeLimit, plus one
of them with several cuts truncated at each of its last 27 bytes, an empty stream and a header-only
one.  Every query runs on a sub-batch view (in_off[0] != 0) with sizes and statuses between 0xA5
guards and the workspace between the guards of tests/dirty.py (the workspace itself starts as 0xA5
unless the caller says otherwise), and must report exactly what
decompressed_sizes(exact_only=True) reports; the stage's counters must add up, equal the first slow
list's length, and show at least the streams with a cut, no stop and status OK as sized by the stage.
The wave route at every chunk size, the lane route and the forced parts route are covered, then
count == 0 and the new call's EINVAL cases.  decompress_batch_sized on 64 streams of 4 segments written
by the oracle's Writer with Reset between its Writes gives the oracle's bytes through the segmented
decode; on a batch without Resets it decodes as before.  All comparisons are exact equality."""

import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import eazy_amd as ez
from k2_streams import HDR
from test_gpu_segments import _guarded, _log_lines, reset_batch  # noqa: F401  (reset_batch: a fixture)
from test_k2_segments import build_check

pytestmark = pytest.mark.gpu

PAD = 37  # bytes before in_off[0]: a sub-batch view


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """[(name, BlockSizeLimit, stream, cuts, stop)] from the host check."""
    tmp = tmp_path_factory.mktemp("k2_segs_size_gpu")
    f = tmp / "streams.bin"
    p = subprocess.run([build_check(tmp), "--dump", str(f)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    raw, at, res = f.read_bytes(), 0, []
    while at < len(raw):
        nname, limit, nb, ncut, stop = struct.unpack_from("<5Q", raw, at)
        at += 40
        name = raw[at : at + nname].decode()
        at += nname
        res.append((name, limit, raw[at : at + nb], ncut, stop))
        at += nb + 16 * ncut
    assert len(res) > 300
    return res


def _truncations(dumped):
    b = next(e[2] for e in dumped if e[1] == 0 and e[3] >= 3 and not e[4])
    return [b[: len(b) - k] for k in range(1, 28)]


def _query(cuda, ins, limit=0, hint=0, in_bytes=False, route="", want_chunk=None, ws_init=0xA5, keep=None):
    """One guarded query and the exact decoder's answer -> (sizes, statuses, (taken, sized, handed on)).
    ws_init: what the workspace holds when the call starts (a fill byte, or a tensor to copy from),
    between its two guards (tests/dirty.py); keep: a list that receives the workspace as the query left it."""
    import torch
    from dirty import guarded, guards_intact

    count = len(ins)
    coff = PAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"\xff" * PAD + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
    comp = comp[: len(comp) - 16]
    d_coff = torch.from_numpy(coff).to(cuda)
    sz_whole, sz = _guarded(cuda, max(count, 1), torch.int64)  # (count == 0: one element, so that the pointers are not NULL)
    st_whole, st = _guarded(cuda, max(count, 1), torch.int32)
    ws_whole, ws = guarded(cuda, ez._lib().ez_decompress_workspace(count), ws_init)
    ez.select_size_route(route)
    try:
        ez.decompressed_sizes(comp, d_coff, block_size_limit=limit, sizes=sz, status=st, workspace=ws, max_len=hint,
                              in_bytes=int(coff[-1] - coff[0]) if in_bytes else 0)
        torch.cuda.synchronize()
        chunk, parts = ez.decompressed_size_chunk_last(), ez.decompressed_size_parts_last()
    finally:
        ez.select_size_route("")
    if want_chunk is not None:
        assert chunk == want_chunk
    if route == "p" and count:
        assert chunk in (256, 1024) and parts[0] > 0, (chunk, parts)
    guards_intact(ws_whole, f"hint {hint}, route {route!r}")
    if keep is not None:
        keep.append(ws.clone())
    for whole, n in ((sz_whole, count), (st_whole, count)):
        raw = whole.view(torch.uint8).cpu().numpy()
        edge = 8 * whole.element_size()
        assert (raw[:edge] == 0xA5).all() and (raw[edge + n * whole.element_size() :] == 0xA5).all()
    counters = ez.decompressed_size_segs_last(ws, count)
    if count == 0:
        return None, None, counters
    xsz, xst = ez.decompressed_sizes(comp, d_coff, block_size_limit=limit, exact_only=True)
    torch.cuda.synchronize()
    sz, st, xsz, xst = sz.cpu().numpy(), st.cpu().numpy(), xsz.cpu().numpy(), xst.cpu().numpy()
    bad = np.flatnonzero((sz != xsz) | (st != xst))
    assert bad.size == 0, (hint, route, bad[:4], sz[bad[:4]], xsz[bad[:4]], st[bad[:4]], xst[bad[:4]])
    taken, sized, handed = counters
    assert taken == sized + handed, counters
    assert taken == int(ws[:4].cpu().numpy().view(np.uint32)[0]), counters  # the first list, as K2z left it
    return sz, st, counters


def _must_size(entries, st):
    """Streams with a cut and no stop (entries: the dump's, None for other streams) whose exact status is OK."""
    return sum(1 for s, e in enumerate(entries) if e is not None and e[3] >= 1 and not e[4] and st[s] == 0)


@pytest.mark.parametrize("hint", [4096, 65536, 1 << 20, 0])
def test_sizes_equal_exact_decoder(cuda, dumped, hint):
    assert ez.decompressed_size_chunk(hint) == {4096: 64, 65536: 256, 1 << 20: 1024, 0: 256}[hint]
    for limit in sorted(set(e[1] for e in dumped)):
        group = [e for e in dumped if e[1] == limit]
        k = min(5, len(group))  # an empty stream and a header-only one among the others
        entries = group[:k] + [None, None] + group[k:]
        ins = [e[2] for e in entries[:k]] + [b"", HDR] + [e[2] for e in group[k:]]
        if limit == 0:
            cut = _truncations(dumped)
            ins += cut
            entries += [None] * len(cut)
        sz, st, (taken, sized, handed) = _query(cuda, ins, limit, hint, want_chunk=ez.decompressed_size_chunk(hint))
        assert (sz[k], st[k]) == (0, 0) and (limit != 0 or (sz[k + 1], st[k + 1]) == (0, 0))  # (the header's 1 MiB window is over a limit)
        must = _must_size(entries, st)
        assert sized >= must and (limit != 0 or must > 250), (sized, must)
        if limit == 0:
            assert (st[-27:] != 0).sum() > 0 and handed >= (st != 0).sum()


def test_lane_route(cuda, dumped):
    short = [e for e in dumped if e[1] == 0 and len(e[2]) <= 4096]
    assert len(short) > 20
    entries = [short[s % len(short)] for s in range(4096)]
    sz, st, (taken, sized, handed) = _query(cuda, [e[2] for e in entries], 0, 4096, want_chunk=1)
    must = _must_size(entries, st)
    assert sized >= must > 1000, (sized, must)


def test_parts_route(cuda, dumped):
    group = [e for e in dumped if e[1] == 0]
    for hint in (65536, 1 << 20):
        sz, st, (taken, sized, handed) = _query(cuda, [e[2] for e in group], 0, hint, in_bytes=True, route="p")
        assert sized >= _must_size(group, st) > 250


def test_count_zero_and_refused_arguments(cuda):
    import torch

    sz, st, counters = _query(cuda, [])
    assert counters == (0, 0, 0)
    L = ez._lib()
    ws = torch.zeros(L.ez_decompress_workspace(4), dtype=torch.uint8, device=cuda)
    c = (C.c_uint64 * 3)(7, 7, 7)
    assert L.ez_decompressed_size_segs_last(None, 4, c) == ez.EINVAL
    assert L.ez_decompressed_size_segs_last(ws.data_ptr(), 4, None) == ez.EINVAL
    assert L.ez_decompressed_size_segs_last(None, 0, None) == ez.EINVAL
    assert L.ez_decompressed_size_segs_last(ws.data_ptr(), 0, c) == ez.OK and list(c) == [0, 0, 0]


def test_sized_decode_of_reset_streams(cuda, reset_batch):
    """64 streams of 4 segments: sized by the stage, decoded segment by segment."""
    import torch

    ins, plain = reset_batch
    coff = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"".join(ins), np.uint8).copy()).to(cuda)
    d_coff = torch.from_numpy(coff).to(cuda)
    ws = torch.zeros(ez._lib().ez_decompress_workspace(64), dtype=torch.uint8, device=cuda)
    need, st0 = ez.decompressed_sizes(comp, d_coff, workspace=ws, max_len=max(len(b) for b in ins))
    torch.cuda.synchronize()
    assert ez.decompressed_size_segs_last(ws, 64) == (64, 64, 0)
    assert need.cpu().tolist() == [len(p) for p in plain] and (st0 == 0).all()
    out, out_off, sizes, status = ez.decompress_batch_sized(comp, d_coff)
    torch.cuda.synchronize()
    assert ez.segments_last()[0] == 256
    assert sizes.cpu().tolist() == [len(p) for p in plain] and (status == 0).all()
    o, oo = out.cpu().numpy(), out_off.cpu().numpy()
    assert all(int(x) % 16 == 0 for x in oo)
    for s, p in enumerate(plain):
        assert o[oo[s] : oo[s] + len(p)].tobytes() == p, s
    # a batch without Resets after output: decompress_batch's decoders, as before
    rng = np.random.default_rng(17)
    import oracle as orc

    texts = [_log_lines(rng, 3000 + 101 * s) for s in range(16)]
    one = [orc.compress(1 << 20, 1024, [t]) for t in texts]
    coff = np.concatenate([[0], np.cumsum([len(b) for b in one])]).astype(np.int64)
    comp = torch.from_numpy(np.frombuffer(b"".join(one), np.uint8).copy()).to(cuda)
    before = ez.segments_last()
    out, out_off, sizes, status = ez.decompress_batch_sized(comp, torch.from_numpy(coff).to(cuda))
    torch.cuda.synchronize()
    assert ez.decompress_kernel_last() in ("r", "t", "j") and ez.segments_last() == before
    assert sizes.cpu().tolist() == [len(t) for t in texts] and (status == 0).all()
    o, oo = out.cpu().numpy(), out_off.cpu().numpy()
    for s, t in enumerate(texts):
        assert o[oo[s] : oo[s] + len(t)].tobytes() == t, s
