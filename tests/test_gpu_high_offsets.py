"""Batch calls with offsets past 2^31 and 2^32: every K1 route, every K2 route and the three queries.

ez_batch's offsets are absolute and 64-bit, a run [a, b) of a batch is itself a batch, and a batch may
be larger than 4 GiB; inside the kernels nearly every position is 32-bit, each route
with its own guard for where that stops being safe.  The route tests put every batch at offset 0 of a
few MiB.  Here the dimension is where the batch lies (tests/high.py):

  A  the hand-built groups of the route tests as views into three buffers of 4 GiB + 64 MiB, at four
     placements (the input across 2^32, the output across 2^32, both above it and unaligned, both
     across 2^31), on the route named and read back from the library's introspection, each held to its
     own test's bar, and every byte of the three buffers outside the batch checked after every call;
  B  the decoders' 32-bit slot limits at their edges: slots of 2^30 - 1, 2^30 and 2^31 + 5 bytes on K2r,
     K2t and K2w, and K2j's pointers 2^32 - 3 and 2^32 - 2 bytes from out_off[0];
  C  two batches that are larger than 4 GiB with in_off[0] == 0: 1,048,583 streams of 4 KiB and 4,163
     of 1 MiB through K1, K3, K2 and the size and Break queries, against the oracle's bytes of one
     period of the input.

The first test runs on the CPU: the placements are what they claim, by arithmetic on the offsets.  The
GPU tests are marked one by one.  All comparisons are exact equality."""

import functools
import time

import numpy as np
import pytest

import high
import k1_inputs as ki
import oracle as orc
from high import PLACEMENTS, T31, T32
from k2_streams import HDR, _need, _oracle, cpy, lit, rb
from test_gpu_dirty_scratch import K2_TARGETS, _jc, _mixed_segments, k2_targets
from test_gpu_k1_edges import GLONG_ROUTES, RING_ROUTES, ROUTE_IDS, ROUTES, named, oracle_bytes

MiB, KiB = 1 << 20, 1 << 10
every_placement = pytest.mark.parametrize("p", PLACEMENTS)
K1_SHORT, K1_LONG = ("A", "E", "G"), ("Glong", "H1024")


# ------------------------------------------------------------------ the CPU proof


def _k1_groups():
    """(what, the routes that run it, block, htable, cases) of every K1 batch of part A."""
    for g in K1_SHORT:
        for ht in (1024, 8192):
            routes = [r[0] for r in ROUTES if r[3] == ht]
            yield f"K1 group {g} htable {ht}", routes, MiB, ht, ki.group(g)
    yield "K1 group Glong", [r[0] for r in GLONG_ROUTES], MiB, 1024, ki.group("Glong")
    h = ki.group("H1024")
    yield "K1 group H1024", [r[2] for r in RING_ROUTES], 1024, h[0].htable, h


def test_placements_are_what_they_claim():
    """CPU.  For every (group, placement), by arithmetic on the offsets alone: the named power of two
    falls strictly inside the batch (so it never coincides with in_off[0]), the side a placement calls
    low ends below 2^31, 'above' is above 2^32 and unaligned, and everything fits the buffers; for
    every route at least one of its groups has the power strictly inside a stream's input or slot, at
    every placement that names one."""
    inside = {}  # {(route, placement): a group of the route has the power inside a stream}
    for what, routes, block, ht, cases in _k1_groups():
        bufs = [c.data for c in cases]
        want = [oracle_bytes(b, block, ht) for b in bufs]
        for p in PLACEMENTS:
            in_off, so = high.k1_layout(p, bufs, want)
            ok, stream = high.claims(p, in_off, so)
            assert ok, (what, p, in_off[[0, -1]], so[[0, -1]])
            for r in routes:
                inside[r, p] = inside.get((r, p), False) or stream
    for name in K2_TARGETS:
        t = k2_targets()[name]
        for p in PLACEMENTS:
            coff, ooff, _ = high.k2_layout(p, t["ins"], t["slots"])
            ok, stream = high.claims(p, coff, ooff)
            assert ok, (name, p, coff[[0, -1]], ooff[[0, -1]])
            for r in (t["kind"], "exact"):
                inside[r, p] = inside.get((r, p), False) or stream
    assert {r for r, _ in inside} == {r[0] for r in ROUTES} | {"r", "t", "w", "j", "exact"}
    for (r, p), stream in inside.items():
        assert stream or high.INSIDE[p] == (None, None), f"route {r} at {p}: no group has the power of two inside a stream"
    # the placements themselves
    assert high.place(PLACEMENTS[0], 1001, 77) == (T32 - 501, 3) and high.place(PLACEMENTS[1], 1001, 78) == (5, T32 - 39)
    assert high.place(PLACEMENTS[2], 1, 1) == (T32 + 5, T32 + 9) and high.place(PLACEMENTS[3], 1000, 10) == (T31 - 501, T31 - 5)


def test_strays_finds_every_byte_outside_the_allowed_intervals():
    """CPU.  high.strays on a small buffer: a changed byte is found in a long gap, in a short one, at a
    gap's first and last byte and at the buffer's ends, and never inside an allowed interval."""
    import torch

    n = 3 * 4096 + 43
    allowed = [(5000, 5003), (100, 164), (5003, 5010), (n - 9, n - 3)]
    for k in (0, 7, 8, 99, 164, 165, 4000, 4999, 5010, 9000, n - 10, n - 3, n - 1):
        buf = torch.full((n,), 0xA5, dtype=torch.uint8)
        buf[k] = 0xA4
        assert high.strays(buf, 0xA5, allowed) == [k], k
        assert high.strays(buf, 0xA5, allowed + [(k, k + 1)]) == []
    buf = torch.full((n,), 0xA5, dtype=torch.uint8)
    for a, b in allowed:
        buf[a:b] = 0
    assert high.strays(buf, 0xA5, allowed) == [] and high.strays(buf, 0xA5, [])[:3] == [100, 101, 102]


# ------------------------------------------------------------------ A: the buffers


@pytest.fixture(scope="module")
def big(cuda):
    import torch

    import eazy_amd as ez

    high.want_memory("A")
    b = high.Big(cuda)
    try:
        yield b
    finally:
        del b.IN, b.SLOTS, b.OUT
        ez.release_cached()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ A: K1


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_k1_views_short_groups(big, route, p):
    """Forward counts (A), runs and zeros (E) and the token writer's widths (G), one batch each, on
    each of the eleven routes at each placement."""
    name, kind, max_len, htable = route
    for g in K1_SHORT:
        assert high.run_k1(big, p, f"group {g}", named(ki.group(g)), MiB, htable, kind, max_len, name) == name


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("route", GLONG_ROUTES, ids=[r[0].replace(" ", "-") for r in GLONG_ROUTES])
def test_k1_views_long_records(big, route, p):
    """G's cases of 4,097 bytes on the six routes that take them."""
    name, kind, max_len, htable = route
    assert high.run_k1(big, p, "group G (long)", named(ki.group("Glong")), MiB, htable, kind, max_len, name) == name


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("kind,max_len,route", RING_ROUTES, ids=[f"{k or 'auto'}-{m}-{r}" for k, m, r in RING_ROUTES])
def test_k1_views_ring(big, kind, max_len, route, p):
    """H at a block of 1,024 bytes (streams of 3 to 9 KiB: the ring's trims and the far skip) on K1L,
    K1x and the general kernel."""
    cases = ki.group("H1024")
    assert high.run_k1(big, p, "group H block 1024", named(cases), 1024, cases[0].htable, kind, max_len, route) == route


# ------------------------------------------------------------------ A: K2


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("name", K2_TARGETS)
def test_k2_views(big, name, p):
    """K2r on R4, R5 and R6, K2t on T6 and T7, K2w on T6, K2j on its three groups: streams handed
    over, literals deferred, damaged streams; the exact decoder runs behind each on the same placement."""
    t = k2_targets()[name]
    kind = t["kind"]
    high.run_k2(big, p, t["ins"], _jc(t["ins"]) if kind == "j" else None, slots=t["slots"], handed=t["handed"], kind=kind,
                max_len=t.get("max_len"), what=name)


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("kind", ["exact"])
def test_k2_views_exact_decoder(big, kind, p):
    """The exact decoder alone (exact_only=True) on R6's mixed wave, T6's deferred literals and
    K2j's copies."""
    for name in ("K2r-R6-mixed-wave", "K2t-T6-deferred", "K2j-copies-handed"):
        t = k2_targets()[name]
        high.run_k2(big, p, t["ins"], slots=t["slots"], kind=kind, max_len=t.get("max_len"), what=name)


# ------------------------------------------------------------------ A: the queries

from test_gpu_breaks import dumped as brk_dumped  # noqa: E402,F401  (fixtures: the host checks' dumped streams)
from test_gpu_segments import dumped as seg_dumped, reset_batch  # noqa: E402,F401
from test_gpu_segments_parts import dumped as parts_dumped, reset_streams  # noqa: E402,F401
from test_gpu_size_segments import dumped as size_dumped  # noqa: E402,F401

QUERY_PLACEMENTS = (PLACEMENTS[0], PLACEMENTS[2], PLACEMENTS[3])  # only in_base matters
query_placement = pytest.mark.parametrize("p", QUERY_PLACEMENTS)

_EXACT = {}


def _exact_sizes(cuda, key, ins):
    """decompressed_sizes(exact_only=True) of the batch at offset 0 of a buffer of its own, once per key."""
    import torch

    import eazy_amd as ez

    if key not in _EXACT:
        comp = torch.from_numpy(np.frombuffer(b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
        coff = torch.from_numpy(high.offsets(0, [len(b) for b in ins])).to(cuda)
        sz, st = ez.decompressed_sizes(comp, coff, exact_only=True)
        torch.cuda.synchronize()
        _EXACT[key] = (sz.cpu().numpy(), st.cpu().numpy())
    return _EXACT[key]


@pytest.mark.gpu
@query_placement
@pytest.mark.parametrize("route", ["lane", "wave", "parts"])
def test_size_query_views(big, size_dumped, route, p):
    """decompressed_sizes on the host check's streams (test_gpu_size_segments.py's batches): the lane
    kernel on 4,096 short ones, the wave kernel and the forced parts route on all of BlockSizeLimit 0.
    Sizes and statuses equal the exact decoder's on the same streams at offset 0; the route is read
    from the chunk and the parts counters."""
    import torch

    import eazy_amd as ez

    if route == "lane":
        short = [e for e in size_dumped if e[1] == 0 and len(e[2]) <= 4096]
        ins = [short[s % len(short)][2] for s in range(4096)]
        hint, sel = 4096, ""
    else:
        ins = [e[2] for e in size_dumped if e[1] == 0]
        hint, sel = 65536, ("p" if route == "parts" else "v")
    want_sz, want_st = _exact_sizes(big.cuda, route == "lane", ins)
    assert (want_st == 0).sum() > len(ins) // 2
    q = high.Query(big, p, ins)
    try:
        sz = torch.full((q.count,), -7, dtype=torch.int64, device=big.cuda)
        st = torch.full((q.count,), -7, dtype=torch.int32, device=big.cuda)
        ws_whole, ws = high.ws_for(big.cuda, ez._lib().ez_decompress_workspace(q.count))
        ez.select_size_route(sel)
        try:
            ez.decompressed_sizes(big.IN, q.d_coff, sizes=sz, status=st, workspace=ws, max_len=hint, in_bytes=q.in_bytes if route == "parts" else 0)
            torch.cuda.synchronize()
            chunk, parts = ez.decompressed_size_chunk_last(), ez.decompressed_size_parts_last()
        finally:
            ez.select_size_route("")
        assert chunk == {"lane": 1, "wave": 256, "parts": 256}[route], chunk
        assert (parts[0] > 0) == (route == "parts"), parts
        from dirty import guards_intact

        guards_intact(ws_whole, f"size query, {route}")
        sz, st = sz.cpu().numpy(), st.cpu().numpy()
        bad = np.flatnonzero((sz != want_sz) | (st != want_st))
        assert bad.size == 0, (route, p, bad[:4], q.coff[bad[:4]], sz[bad[:4]], want_sz[bad[:4]], st[bad[:4]], want_st[bad[:4]])
        taken, sized, handed = ez.decompressed_size_segs_last(ws, q.count)
        assert taken == sized + handed and sized > 20, (taken, sized, handed)
    finally:
        q.done(f"size query, {route} route")


def _segment_query(big, q, group, route, max_len):
    """ez_stream_segments_batch on the placed batch under a route -> the arrays equal the host walk's."""
    import ctypes as C

    import torch

    import eazy_amd as ez
    from dirty import guards_intact
    from test_gpu_segments_parts import _expected

    idx, sin, sout = _expected(group, q.coff, q.ooff)
    found, count = int(idx[-1]), q.count
    cap = found + 3
    a5 = int(np.frombuffer(b"\xa5" * 8, np.int64)[0])
    arrs = [torch.full((n,), a5, dtype=torch.int64, device=big.cuda) for n in (count + 1, cap + 1, cap + 1, 2)]
    ws_whole, ws = high.ws_for(big.cuda, ez._lib().ez_segments_workspace(count))
    b = ez._Batch(big.IN.data_ptr(), q.d_coff.data_ptr(), None, q.d_ooff.data_ptr(), None, None, count, max_len, q.in_bytes if route == "p" else 0, 0)
    ez.select_segments_route(route)
    try:
        st = ez._lib().ez_stream_segments_batch(0, C.byref(b), arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(), cap, arrs[3].data_ptr(),
                                                ws.data_ptr(), ez._stream_ptr(None))
        assert st == ez.OK, st
        torch.cuda.synchronize()
        last = ez.segments_parts_last()
    finally:
        ez.select_segments_route("")
    guards_intact(ws_whole, "the segment query")
    assert (last[0] > 0) == (route == "p"), (route, last)
    seg_idx, seg_in, seg_out, total = (a.cpu().numpy() for a in arrs)
    assert tuple(total) == (found, found)
    bad = np.flatnonzero(seg_idx != idx)
    assert bad.size == 0, (group[int(bad[0]) - 1][0], seg_idx[bad[:4]], idx[bad[:4]])
    for nm, got, want in (("seg_in", seg_in[: found + 1], sin), ("seg_out", seg_out[: found + 1], sout)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (nm, group[int(np.searchsorted(idx, bad[0], "right")) - 1][0], got[bad[:4]], want[bad[:4]])
    assert (seg_in[found + 1 :] == a5).all() and (seg_out[found + 1 :] == a5).all()


@pytest.mark.gpu
@query_placement
@pytest.mark.parametrize("route", ["wave", "parts"])
def test_segment_query_views(big, seg_dumped, parts_dumped, route, p):
    """stream_segments: the wave route on test_gpu_segments.py's streams and the forced parts route on
    test_gpu_segments_parts.py's long ones (BlockSizeLimit 0), with slots that clamp every fifth
    stream's cuts: seg_idx, seg_in and seg_out equal the host walk's, in absolute offsets."""
    from test_gpu_segments_parts import _caps

    group = [e for e in (seg_dumped if route == "wave" else parts_dumped) if e[1] == 0]
    if route == "parts":
        group = group[:2] + [("empty", 0, b"", [])] + group[2:]
    q = high.Query(big, p, [e[2] for e in group], _caps(group))
    try:
        _segment_query(big, q, group, "v" if route == "wave" else "p", 0)
    finally:
        q.done(f"segment query, {route} route")


@pytest.mark.gpu
@every_placement
@pytest.mark.parametrize("route", ["wave", "parts"])
def test_segmented_decode_views(big, seg_dumped, reset_batch, reset_streams, route, p):
    """decompress_batch_segmented: under the wave route on test_gpu_segments.py's mixed batch (valid
    4-segment streams, an error in segment 2 of 4, plain and empty streams), under the forced parts
    route on 8 oracle-written streams of 20 segments."""
    from k2_streams import _slot

    if route == "wave":
        ins = _mixed_segments(seg_dumped, reset_batch)
        caps = [_slot(s, _need(b)) for s, b in enumerate(ins)]
        sz, st, segs, parts = high.run_segmented(big, p, ins, caps, "v")
        assert sorted(np.flatnonzero(st != 0)) == [2, 3, 4] and segs[0] == 5 * 4 + 3 * 3 + 3 + 2 and segs[1] >= 3
        assert parts == (0, 0, 0, 0)
    else:
        ins, plain = reset_streams
        sz, st, segs, parts = high.run_segmented(big, p, ins, [len(t) + 1 + s % 5 for s, t in enumerate(plain)], "p")
        # (the decode's query runs in the decode's own scratch, whose parts counters the library does not report:
        # segments_parts_last is the stand-alone query's, asserted in test_segment_query_views)
        assert not st.any() and list(sz) == [len(t) for t in plain] and segs[:2] == (160, 0)


@pytest.mark.gpu
@query_placement
@pytest.mark.parametrize("max_len", [4096, 1 << 20])
def test_break_query_views(big, brk_dumped, max_len, p):
    """stream_breaks on the host check's streams of BlockSizeLimit 0 at the smallest and the largest
    chunk: brk_idx, brk_pos, sizes and statuses are the oracle Reader's; the walk ran (it hands the
    streams with an error to the exact decoder, and few others)."""
    import torch

    import eazy_amd as ez
    from dirty import guards_intact
    from test_gpu_breaks import _expected

    group = [e for e in brk_dumped if e[1] == 0]
    idx, pos, wsz, wst = _expected(group)
    found = int(idx[-1])
    assert found > 1000 and (wst != 0).sum() > 0
    q = high.Query(big, p, [e[2] for e in group])
    try:
        ws_whole, ws = high.ws_for(big.cuda, ez._lib().ez_breaks_workspace(q.count))
        brk_idx, brk_pos, sizes, status = ez.stream_breaks(big.IN, q.d_coff, max_len=max_len, brk_cap=found + 3, workspace=ws)
        torch.cuda.synchronize()
        guards_intact(ws_whole, "the break query")
        for name, a, w in (("brk_idx", brk_idx, idx), ("out_size", sizes, wsz), ("status", status, wst), ("brk_pos", brk_pos[:found], pos)):
            a = a.cpu().numpy()
            bad = np.flatnonzero(a != w)
            assert bad.size == 0, (name, p, bad[:4], a[bad[:4]], w[bad[:4]])
        w = ws.cpu().numpy().view(np.uint32)
        listed = set(w[16 : 16 + int(w[15])].tolist())
        assert set(np.flatnonzero(wst != 0).tolist()) <= listed and len(listed) < q.count, (len(listed), q.count)
    finally:
        q.done("break query")


# ------------------------------------------------------------------ B: the 32-bit slot limits


B_SLOTS = (64, (1 << 30) - 1, 1 << 30, 64, (1 << 31) + 5, 64)


@functools.lru_cache(maxsize=None)
def _b_streams():
    """Six streams of about 40 bytes: a literal, a near copy, a far copy."""
    rng = np.random.default_rng(3230)
    return tuple(HDR + lit(rb(rng, 24 + s)) + cpy(3, 9 + s) + cpy(20 + s, 8) for s in range(6))


@pytest.mark.gpu
@pytest.mark.parametrize("hints", ["no-extents", "extents"])
@pytest.mark.parametrize("max_len", ["max_len-exact", "max_len-0"])
@pytest.mark.parametrize("kind", ["r", "t", "w"])
def test_slot_limits(big, kind, max_len, hints):
    """Slots of 64, 2^30 - 1, 2^30, 64, 2^31 + 5 and 64 bytes in OUT, about 4 GiB of offsets and a few
    hundred bytes written: every stream gives the oracle's bytes, size and status 0; the decoder hands
    over exactly streams 2 and 4, whose slots are 2^30 bytes or more, and takes the one of 2^30 - 1;
    the three 64-byte neighbours and all slack are untouched.  With max_len stated exactly and with 0
    (measured on the device, where the maximum saturates at 2^32 - 1), with the extent hints and without."""
    ins = list(_b_streams())
    for b in ins:
        assert _oracle(b, 64)[1] == 0 and 30 < _need(b) < 64
    cap = list(B_SLOTS)
    coff, ooff = high.offsets(11, [len(b) for b in ins]), high.offsets(5, cap)
    assert ooff[2] < T31 < ooff[3] and ooff[4] < T32 < ooff[5] and ooff[-1] + 64 <= high.SPAN
    ext = (lambda nin, nout: dict(in_bytes=nin, out_bytes=nout)) if hints == "extents" else None
    got = high.run_k2(big, "low", ins, handed={2, 4}, kind=kind, max_len=True if max_len == "max_len-exact" else 0, hints=ext,
                      layout=(coff, ooff, cap), what="slot limits")
    assert got == {2, 4}


@functools.lru_cache(maxsize=None)
def _kj_streams():
    """Four log inputs of 256 KiB decoded each, as the oracle's Writer compresses them."""
    from eazy_amd import synth

    d = synth.logs(3231, 4 << 18).tobytes()
    plain = [d[k << 18 : (k + 1) << 18] for k in range(4)]
    return [orc.compress(MiB, 1024, [t]) for t in plain], plain


# (inputs, out_off[s + 1] - out_off[0] of each, the streams K2j must hand over): one batch cannot hold slots of
# 256 KiB that end at 2^32 - 3, 2^32 - 2 and 2^32 + 64 KiB, so each of the three ends has a batch of its own, the
# first input (slot end 2^20, always taken) in front
K2J_BATCHES = (((0, 1), (1 << 20, T32 - 3), set()), ((0, 2), (1 << 20, T32 - 2), {1}), ((0, 3), (1 << 20, T32 + 64 * KiB), {1}))


@pytest.mark.gpu
def test_k2j_pointer_limit(cuda):
    """K2j keeps 32-bit pointers relative to out_off[0] (rounded down to 16 bytes; here it is aligned):
    four log streams of 256 KiB decoded whose slots end 2^20, 2^32 - 3, 2^32 - 2 and 2^32 + 64 KiB bytes
    from out_off[0], the last three each in a batch of its own behind the first.  The first two are
    taken, the last two handed over; bytes, sizes and statuses are the oracle's.  (The pointer array
    spans the batch's output extent: about 17 GiB of scratch per batch, cleared and walked by the
    pointer passes.)"""
    import torch

    import eazy_amd as ez

    high.want_memory("B-K2j")
    ins_all, plain_all = _kj_streams()
    assert all(2 * len(b) < len(t) for b, t in zip(ins_all, plain_all))
    lead = 16
    out = None
    try:
        out = torch.full((lead + T32 + 64 * KiB + 64,), high.FILL, dtype=torch.uint8, device=cuda)
        for which, ends, handed in K2J_BATCHES:
            ins, plain, count = [ins_all[k] for k in which], [plain_all[k] for k in which], len(which)
            ooff = np.array([lead] + [lead + e for e in ends], np.int64)
            coff = high.offsets(3, [len(b) for b in ins])
            assert all(len(plain[s]) <= ooff[s + 1] - ooff[s] < T32 - 2 for s in range(count))
            comp = torch.from_numpy(np.frombuffer(b"\xff" * 3 + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
            sz = torch.full((count,), -7, dtype=torch.int64, device=cuda)
            st = torch.full((count,), -7, dtype=torch.int32, device=cuda)
            ws = torch.full((ez._lib().ez_decompress_workspace(count),), 0xA5, dtype=torch.uint8, device=cuda)
            d_coff, d_ooff = torch.from_numpy(coff).to(cuda), torch.from_numpy(ooff).to(cuda)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ez.select_decompress_kernel("j")
            try:
                ez.decompress_batch(comp, d_coff, d_ooff, out=out, sizes=sz, status=st, workspace=ws)
                torch.cuda.synchronize()
                took = ez.decompress_kernel_last()
            finally:
                ez.select_decompress_kernel("")
            print(f"K2j over a span of {int(ooff[-1] - ooff[0])} bytes: {time.perf_counter() - t0:.2f} s")
            assert took == "j", took
            w = ws[: 4 * (count + 1)].cpu().numpy().view(np.uint32)
            assert set(w[1 : 1 + min(int(w[0]), count)].tolist()) == handed and int(w[0]) == len(handed), (ends, w)
            assert sz.cpu().tolist() == [len(t) for t in plain] and not st.cpu().numpy().any(), (ends, sz, st)
            may = []
            for s, t in enumerate(plain):
                o = int(ooff[s])
                assert out[o : o + len(t)].cpu().numpy().tobytes() == t, f"ends {ends}: stream {s} differs from the oracle's"
                may.append((o, o + len(t)))
            assert high.strays(out, high.FILL, may) == [], f"ends {ends}: bytes outside the outputs written"
            for a, b in may:
                out[a:b].fill_(high.FILL)
    finally:
        out = None
        ez.release_cached()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ C: batches larger than 4 GiB


def _tiled(cuda, region, lens_period, count):
    """-> (data, in_off, lens) on the device: `count` streams whose lengths and bytes repeat with the
    period len(lens_period); one period's streams lie back to back in region[: sum(lens_period)]."""
    import torch

    period = len(lens_period)
    P = int(np.sum(lens_period))
    reps, rest = divmod(count, period)
    tail = int(np.sum(lens_period[:rest]))
    reg = torch.from_numpy(region[:P]).to(cuda)
    data = torch.empty(reps * P + tail + 16, dtype=torch.uint8, device=cuda)
    data[: reps * P].view(reps, P).copy_(reg.expand(reps, P))
    data[reps * P : reps * P + tail].copy_(reg[:tail])
    lens = torch.from_numpy(np.asarray(lens_period, np.int64)).to(cuda).repeat(reps + 1)[:count]
    in_off = torch.zeros(count + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(lens, 0, out=in_off[1:])
    return data[: reps * P + tail], in_off, lens


def _oracle_period(region, lens_period):
    """The oracle's compressed bytes of one period's streams -> (their bytes back to back, their sizes)."""
    offs = np.concatenate([[0], np.cumsum(lens_period)]).astype(np.int64)
    caps = np.asarray(lens_period, np.int64) + (np.asarray(lens_period, np.int64) >> 2) + 64
    slot_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    slots, sizes = orc.compress_batch(MiB, 1024, region[: int(offs[-1])], offs, slot_off, 16)
    sizes = np.asarray(sizes, np.int64)
    keep = np.concatenate([slots[int(slot_off[s]) : int(slot_off[s]) + int(sizes[s])] for s in range(len(sizes))])
    return keep, sizes


def _larger_than_4gib(cuda, what, region, lens_period, count, last_len, max_len, k1_routes, k2_route):
    """K1 (on each of k1_routes: (forced kind, route)), K3, K2 and the size and Break queries on `count` tiled streams, compared on the
    device with the oracle's result of one period.  last_len: the last stream is cut to this length
    (None: the pattern's)."""
    import torch

    import eazy_amd as ez

    period = len(lens_period)
    want_bytes, want_sizes = _oracle_period(region, lens_period)
    t0 = time.perf_counter()
    data, in_off, lens = _tiled(cuda, region, lens_period, count)
    last_want = None
    if last_len is not None:
        j = (count - 1) % period
        a = int(np.sum(lens_period[:j]))
        last_want = np.frombuffer(orc.compress(MiB, 1024, [region[a : a + last_len].tobytes()]), np.uint8)
        lens[-1] = last_len
        in_off[-1] = in_off[-2] + last_len
        data = data[: int(in_off[-1])]
    total_in = int(in_off[-1])
    # the expected sizes and packed offsets, tiled
    wsz = torch.from_numpy(want_sizes).to(cuda).repeat(count // period + 1)[:count].clone()
    if last_want is not None:
        wsz[-1] = len(last_want)
    wpoff = torch.zeros(count + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(wsz, 0, out=wpoff[1:])
    d_want = torch.from_numpy(want_bytes).to(cuda)
    per = int(want_sizes.sum())
    slot_off = ez.slot_offsets(in_off)
    assert int(slot_off[-1]) > T32 and int(in_off[0]) == 0
    packed = poff = None
    for kind, route in k1_routes:
        ez.select_compress_kernel(kind)
        try:
            cb = ez.compress_batch(data, in_off, MiB, 1024, max_len=max_len, slot_off=slot_off)
            torch.cuda.synchronize()
            took = ez.compress_route_last()
        finally:
            ez.select_compress_kernel("")
        assert took == route, f"{what}: K1 took {took!r}, expected {route!r}"
        assert int(cb.status.count_nonzero()) == 0
        bad = torch.nonzero(cb.sizes != wsz)[:4, 0].tolist()
        assert not bad, f"{what} on {took}: the sizes of streams {bad} differ from the oracle's: {cb.sizes[bad].tolist()}, {wsz[bad].tolist()}"
        packed = torch.empty(int(wpoff[-1]) + 16, dtype=torch.uint8, device=cuda)
        poff = torch.empty(count + 1, dtype=torch.int64, device=cuda)
        ez.pack(cb, packed, poff)
        torch.cuda.synchronize()
        assert torch.equal(poff, wpoff), f"{what} on {took}: packed_off is not the 64-bit cumsum of the sizes"
        for k in range(0, count, period):
            a, n = int(wpoff[k]), min(period, count - k)
            b = int(wpoff[k + n])
            if last_want is not None and k + n == count:
                b = int(wpoff[count - 1])
                assert torch.equal(packed[b : b + len(last_want)], torch.from_numpy(last_want.copy()).to(cuda)), f"{what} on {took}: the last stream differs"
            assert b - a <= per and torch.equal(packed[a:b], d_want[: b - a]), f"{what} on {took}: streams {k} .. {k + n - 1} differ from the oracle's bytes"
        del cb
    # K2 into slots of the input's length plus 16 bytes: out_off passes 2^32 where in_off may not
    out_off = in_off + 16 * torch.arange(count + 1, dtype=torch.int64, device=cuda)
    assert int(out_off[-1]) > T32
    out = torch.full((int(out_off[-1]) + 16,), high.FILL, dtype=torch.uint8, device=cuda)
    _, dsz, dst = ez.decompress_batch(packed, poff, out_off, out=out, max_len=max_len + 16)
    torch.cuda.synchronize()
    assert ez.decompress_kernel_last() == k2_route, ez.decompress_kernel_last()
    assert int(dst.count_nonzero()) == 0 and torch.equal(dsz, lens), f"{what}: decoded sizes"
    period_bytes = int(np.sum(lens_period))
    if len(set(lens_period.tolist())) == 1:
        n = int(lens_period[0])
        full = count - (1 if last_len is not None else 0)
        rows = out[: full * (n + 16)].view(full, n + 16)
        for k in range(0, full, 1024):  # (1 GiB of rows at a time: the comparison's temporary stays small)
            assert torch.equal(rows[k : k + 1024, :n].reshape(-1), data[k * n : min(k + 1024, full) * n]), f"{what}: the decoded bytes of streams {k} .. are not the input"
        assert bool((rows[:, n:] == high.FILL).all()), f"{what}: slack written"
        if last_len is not None:
            o = full * (n + 16)
            assert torch.equal(out[o : o + last_len], data[full * n :]), f"{what}: the last stream's decoded bytes are not the input"
            assert bool((out[o + last_len : o + last_len + 32] == high.FILL).all()), f"{what}: slack written after the last stream"
    else:
        # ragged: gather the outputs period by period through an index built once
        o_per = (out_off[:period] - out_off[0]).cpu().numpy()
        idx = torch.from_numpy(np.concatenate([np.arange(int(o), int(o) + int(n)) for o, n in zip(o_per, lens_period)]).astype(np.int64)).to(cuda)
        gap = torch.from_numpy(np.concatenate([np.arange(int(o) + int(n), int(o) + int(n) + 16) for o, n in zip(o_per, lens_period)]).astype(np.int64)).to(cuda)
        stride = period_bytes + 16 * period
        for k in range(0, count - period + 1, period):
            base = k // period * stride
            assert torch.equal(out[base : base + stride][idx], data[:period_bytes]), f"{what}: the decoded bytes of streams {k} .. differ from the input"
            assert bool((out[base : base + stride][gap] == high.FILL).all()), f"{what}: slack written after streams {k} .."
        k = count // period * period
        for s in range(k, count):
            o, n, a = int(out_off[s]), int(lens[s]), int(in_off[s])
            assert torch.equal(out[o : o + n], data[a : a + n]) and bool((out[o + n : o + n + 16] == high.FILL).all()), (what, s)
    del out
    # the queries on the packed batch
    sz, st = ez.decompressed_sizes(packed, poff, max_len=int(want_sizes.max()))
    torch.cuda.synchronize()
    assert int(st.count_nonzero()) == 0 and torch.equal(sz, lens), f"{what}: decompressed_sizes"
    brk_idx, brk_pos, bsz, bst = ez.stream_breaks(packed, poff, max_len=int(want_sizes.max()), brk_cap=16)
    torch.cuda.synchronize()
    assert int(brk_idx.count_nonzero()) == 0 and int(bst.count_nonzero()) == 0 and torch.equal(bsz, lens), f"{what}: stream_breaks"
    print(f"{what}: {count} streams, {total_in} bytes in, {int(wpoff[-1])} packed: {time.perf_counter() - t0:.2f} s after the oracle")


def _part_c(cuda, run):
    import torch

    import eazy_amd as ez

    high.want_memory("C")
    try:
        run()
    finally:
        ez.release_cached()
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_c_short_batch_larger_than_4gib(cuda):
    """1,048,583 streams whose lengths repeat with a period of 16,384: 4,096 bytes mostly, 4,093 where
    s % 7 == 0, none where s % 4099 == 0 (s within the period), cut back to back from 64 MiB of logs, so
    the offsets are not 16-aligned.  The compress slots (5.4 GB) and the decode's slots (the length
    plus 16 bytes) pass 2^32; the input itself ends 1.5 MB short of it (the lengths under 4,096 take
    that much from 2^20 + 7 streams of 4 KiB).  Automatic routes: s:lean g16 fw40, K3, K2r."""
    from eazy_amd import synth

    j = np.arange(16384)
    lens = np.where(j % 4099 == 0, 0, np.where(j % 7 == 0, 4093, 4096)).astype(np.int64)
    region = synth.logs(3232, 64 << 20)
    _part_c(cuda, lambda: _larger_than_4gib(cuda, "C-short", region, lens, 1_048_583, None, 4096, [("", "s:lean g16 fw40")], "r"))


@pytest.mark.gpu
def test_c_long_batch_larger_than_4gib(cuda):
    """4,163 streams of 1 MiB from 64 MiB of logs (a period of 64), the last one 1 MiB - 4,097 bytes:
    in_off passes 2^32 at stream 4,096.  A max_len of 1 MiB takes K1x (test_gpu_k1_hints.C1_ROUTES),
    whose rounds leave the rest to K1L; K1L alone (forced, every stream through count * rec_cap
    records of 16 bytes, 11.6 GB) runs second; then K3, K2t and the queries."""
    from eazy_amd import synth

    lens = np.full(64, MiB, np.int64)
    region = synth.logs(3233, 64 << 20)
    _part_c(cuda, lambda: _larger_than_4gib(cuda, "C-long", region, lens, 4163, MiB - 4097, MiB, [("", "x"), ("l", "l")], "t"))
