"""K2b's parts route on the GPU (ez_decompress_brk_parts.hip): the Break index of long streams cut over
many waves, forced with ez_select_breaks_route('p') and given b->in_bytes.

The query runs on the hand-built streams of the host check (tools/k2_brk_parts_check.hip, which writes
them with the oracle Reader's size, status and Break positions and, per chunk size, whether the route
takes each stream, its parts and its parts that hold a Break, with --dump) at both chunk sizes, on a
sub-batch view (bytes before in_off[0]), every output array and the workspace between 0xA5 guards,
after the library's cached scratch was filled with 0xA5: its arrays equal the Reader's, the wave
route's ('v') and the call's without a workspace.  The route's counters, the in_bytes hint (under-stated
by 1, unknown, over-stated three times), the room (brk_cap = found, found - 1, 0 with brk_pos NULL, no
Break, count == 0), 8 streams of 256 KiB of log text written by the oracle's Writer with a Break after
every message, more than 64 streams, and the call order on scratch left by itself, by a forced segment
query and by a forced size query follow.  All comparisons are exact equality."""

import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import eazy_amd as ez
import oracle as orc
from test_k2_brk_parts import build_check

pytestmark = pytest.mark.gpu

PAD = 37  # bytes before in_off[0]: a sub-batch view
A5_64 = int(np.frombuffer(b"\xa5" * 8, np.int64)[0])
A5_32 = int(np.frombuffer(b"\xa5" * 4, np.int32)[0])
CHUNK = {0: 256, 1 << 20: 1024}  # max_len -> the parts route's chunk
TEN = b"\x80\x02eazy\x80\x10\x14\x00"


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """[(name, BlockSizeLimit, stream, size, status, [positions], {chunk: (taken, parts, parts holding a Break)})]
    from the host check."""
    tmp = tmp_path_factory.mktemp("k2_brk_parts_gpu")
    f = tmp / "streams.bin"
    p = subprocess.run([build_check(tmp), "--dump", str(f)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    raw, at, res = f.read_bytes(), 0, []
    while at < len(raw):
        h = struct.unpack_from("<12Q", raw, at)
        at += 96
        nname, limit, nb, nbrk, size, status = h[:6]
        name = raw[at : at + nname].decode()
        at += nname
        b = raw[at : at + nb]
        at += nb
        pos = list(struct.unpack_from(f"<{nbrk}Q", raw, at))
        at += 8 * nbrk
        res.append((name, limit, b, size, status, pos, {256: h[6:9], 1024: h[9:12]}))
    assert len(res) > 80 and sum(len(e[5]) for e in res) > 10000
    assert sum(1 for e in res if e[4] != 0 and e[5]) >= 10  # (the errors in the middle, built with Breaks before them)
    return res


def _groups(dumped):
    """per BlockSizeLimit: the dumped streams with an empty and a 10-byte stream among them"""
    for limit in sorted(set(e[1] for e in dumped)):
        group = [e for e in dumped if e[1] == limit]
        none = {256: (1, 0, 0), 1024: (1, 0, 0)}
        group.insert(2, ("empty", limit, b"", 0, 0, [], none))
        ten = TEN if limit == 0 else TEN[:8] + b"\x10\x00"  # (a window within the BlockSizeLimit)
        group.insert(5, ("ten bytes", limit, ten, 0, 0, [], {256: (1, 1, 0), 1024: (1, 1, 0)}))
        yield limit, group


def _guarded(cuda, n, dtype):
    """A tensor of n elements between two guards of 8 elements, everything 0xA5 bytes."""
    import torch

    whole = torch.full(((n + 16) * dtype.itemsize,), 0xA5, dtype=torch.uint8, device=cuda).view(dtype)
    return whole, whole[8 : 8 + n]


_INPUTS = {}


def _inputs(cuda, ins):
    """The batch on the device, once per list of streams -> (comp, d_coff, in_bytes)."""
    import torch

    key = tuple(id(b) for b in ins)
    if key not in _INPUTS:
        coff = PAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
        comp = torch.from_numpy(np.frombuffer(b"\xff" * PAD + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
        _INPUTS[key] = (ins, comp[: len(comp) - 16], torch.from_numpy(coff).to(cuda), int(coff[-1] - coff[0]))
    return _INPUTS[key][1:]


def _query(cuda, ins, cap, limit=0, max_len=0, in_bytes=None, route="p", use_ws=True, null_pos=False, stream=None, dirty=True):
    """ez_stream_breaks_batch under a route, on 0xA5 scratch, into guarded arrays -> ((brk_idx, brk_pos,
    sizes, status, brk_total) as numpy, brk_pos whole (cap entries), the route's counters); the guards
    are checked.  in_bytes None: the exact extent.  dirty False: the cached scratch stays as the last call left it."""
    import torch
    from dirty import guarded, guards_intact

    L = ez._lib()
    count = len(ins)
    comp, d_coff, extent = _inputs(cuda, ins)
    arrs = [_guarded(cuda, n, dt) for n, dt in ((count + 1, torch.int64), (cap, torch.int64), (count, torch.int64), (count, torch.int32), (2, torch.int64))]
    ws_whole, ws = guarded(cuda, L.ez_breaks_workspace(count), 0xA5)
    ptr = [whole.data_ptr() + 8 * whole.element_size() for whole, _ in arrs]  # (an empty view has no address of its own)
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, ptr[2], ptr[3], count, max_len, extent if in_bytes is None else in_bytes, 0)
    ez.select_breaks_route(route)
    try:
        if dirty:
            ez.fill_cached(0xA5)
        torch.cuda.synchronize()
        st = L.ez_stream_breaks_batch(limit, C.byref(b), ptr[0], None if null_pos else ptr[1], cap, ptr[4], ws.data_ptr() if use_ws else None,
                                      ez._stream_ptr(stream))
        assert st == ez.OK, st
        torch.cuda.synchronize()
        last = ez.breaks_parts_last()
    finally:
        ez.select_breaks_route("")
    out = []
    for whole, view in arrs:
        w, a5 = whole.cpu().numpy(), A5_64 if whole.dtype == torch.int64 else A5_32
        assert (w[:8] == a5).all() and (w[-8:] == a5).all()
        out.append(view.cpu().numpy())
    guards_intact(ws_whole, "the break query")
    return out, last


def _expected(group):
    idx = np.concatenate([[0], np.cumsum([len(e[5]) for e in group])]).astype(np.int64)
    pos = np.array([p for e in group for p in e[5]], dtype=np.int64)
    return idx, pos, np.array([e[3] for e in group], dtype=np.int64), np.array([e[4] for e in group], dtype=np.int32)


def _assert_equals(group, got, want, cap):
    brk_idx, brk_pos, sizes, status, total = got
    idx, pos, wsz, wst = want
    found = int(idx[-1])
    assert found <= cap and tuple(total) == (found, found)
    for name, a, w in (("brk_idx", brk_idx[1:], idx[1:]), ("out_size", sizes, wsz), ("status", status, wst)):
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, (name, group[int(bad[0])][0], a[bad[:4]], w[bad[:4]])
    assert brk_idx[0] == 0
    bad = np.flatnonzero(brk_pos[:found] != pos)
    assert bad.size == 0, (group[int(np.searchsorted(idx, bad[0], "right")) - 1][0], bad[:4], brk_pos[bad[:4]], pos[bad[:4]])
    assert (brk_pos[found:] == A5_64).all()


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:4])


@pytest.mark.parametrize("max_len", [0, 1 << 20])
def test_query_equals_oracle_reader_and_wave_route(cuda, dumped, max_len):
    chunk = CHUNK[max_len]
    assert ez._lib().ez_decompressed_size_chunk(max_len) == chunk
    for limit, group in _groups(dumped):
        ins = [e[2] for e in group]
        want = _expected(group)
        cap = int(want[0][-1]) + 3
        got, last = _query(cuda, ins, cap, limit, max_len)
        _assert_equals(group, got, want, cap)
        wave, wlast = _query(cuda, ins, cap, limit, max_len, route="v")
        _same(got, wave, "parts against the wave route")
        assert wlast == (0, 0, 0, 0)
        exact, xlast = _query(cuda, ins, cap, limit, max_len, use_ws=False)
        _same(got, exact, "parts against the call without a workspace")
        assert xlast == (0, 0, 0, 0)
        # the counters: every part in the first pass; records taken and parts walked again; the fill stages
        # exactly the parts that hold a Break, of the streams the route takes
        parts = sum(e[6][chunk][1] for e in group)
        holding = sum(e[6][chunk][2] for e in group if e[6][chunk][0])
        assert parts == sum(-(-len(b) // (64 * chunk)) for b in ins) and (holding > 0 or limit != 0)
        assert last[0] == parts and last[1] + last[2] > 0 and last[3] == holding, (last, parts, holding)
        # the hint: under-stated by 1 (the wave route walks the batch: counters 0), unknown, over-stated three times
        extent = _inputs(cuda, ins)[2]
        for hint, ran in ((extent - 1, False), (0, False), (3 * extent, True)):
            again, hlast = _query(cuda, ins, cap, limit, max_len, in_bytes=hint)
            _same(got, again, f"in_bytes {hint}")
            assert hlast == (last if ran else (0, 0, 0, 0)), (hint, hlast)


def test_adversarial_bodies_are_walked_again(cuda, dumped):
    group = [e for e in dumped if "in literal bodies" in e[0] and e[1] == 0]
    assert len(group) >= 20
    ins = [e[2] for e in group]
    want = _expected(group)
    cap = int(want[0][-1])
    for max_len in CHUNK:
        got, last = _query(cuda, ins, cap, 0, max_len)
        _assert_equals(group, got, want, cap)
        assert last[2] > 0 and last[0] == sum(e[6][CHUNK[max_len]][1] for e in group), last


def test_room(cuda, dumped):
    limit, group = next(_groups(dumped))
    group = [e for e in group if e[0].startswith("C256 ") or not e[2] or e[2] == TEN][:60]
    ins = [e[2] for e in group]
    want = _expected(group)
    found = int(want[0][-1])
    assert found > 5000
    got, last = _query(cuda, ins, found, limit)  # brk_cap = found writes everything
    _assert_equals(group, got, want, found)
    assert last[3] > 0
    for cap, null_pos in ((found - 1, False), (0, True), (0, False)):
        (brk_idx, brk_pos, sizes, status, total), last = _query(cuda, ins, cap, limit, null_pos=null_pos)
        assert tuple(total) == (0, found) and last[0] > 0 and last[3] == 0, (total, last)
        assert np.array_equal(brk_idx, want[0]) and np.array_equal(sizes, want[2]) and np.array_equal(status, want[3])
        assert (brk_pos == A5_64).all()
    # a batch without any Break: the oracle Writer's streams of 40,000 and 20,000 random bytes, and the ten bytes
    rng = np.random.default_rng(31)
    plain = []
    for n in (40000, 0, 20000):
        w = orc.Writer(1 << 20, 1024)
        text = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert n == 0 or w.write(text) == (n, 0)
        plain.append(w.sink if n else TEN)
        assert orc.decompress(plain[-1])[:2] == (text, 0)
    (brk_idx, brk_pos, sizes, status, total), last = _query(cuda, plain, 5)
    assert tuple(total) == (0, 0) and not brk_idx.any() and (brk_pos == A5_64).all() and not status.any()
    assert list(sizes) == [40000, 0, 20000]
    assert last[0] == sum(-(-len(b) // (64 * 256)) for b in plain) >= 5 and last[3] == 0, last
    # count == 0
    (brk_idx, brk_pos, sizes, status, total), last = _query(cuda, [], 4)
    assert list(brk_idx) == [0] and tuple(total) == (0, 0) and (brk_pos == A5_64).all() and last == (0, 0, 0, 0)


def _log_lines(rng, n):
    out = bytearray()
    while len(out) < n:
        out += b"2026-01-01T00:00:%02d INFO tenant-%d GET /api/v1/items/%d status=200 bytes=%d\n" % (
            rng.integers(60), rng.integers(13), rng.integers(5000), rng.integers(100000))
    return bytes(out[:n])


def _reader_breaks(comp):
    """The oracle Reader on comp read to EOF -> (output, [bytes produced at each ErrBreak], error)."""
    r = orc.Reader(b=comp)
    out, pos = b"", []
    while True:
        got, err = r.read(1 << 16)
        out += got
        if err == 10:  # ErrBreak
            pos.append(len(out))
            continue
        if err != 0 or not got:
            return out, pos, 0 if err == 1 else err


@pytest.fixture(scope="module")
def written():
    """8 streams by the oracle's Writer: 256 KiB of log text each, write_break after every message, a
    Reset every 64 KiB -> (streams, messages per stream as the Breaks delimit them, the Reader's positions)."""
    rng = np.random.default_rng(29)
    ins, msgs, poss = [], [], []
    for s in range(8):
        w = orc.Writer(1 << 20, 1024)
        mine, done, resets = [], 0, 0
        if s == 5:  # starts with a Break: an empty first message
            assert w.write_break() == 0
            mine.append(b"")
        k = 0
        while done < (256 << 10):
            if done // (64 << 10) > resets:
                w.reset()
                resets += 1
            m = _log_lines(rng, 300 + int(rng.integers(1500)))
            assert w.write(m) == (len(m), 0)
            assert w.write_break() == 0
            mine.append(m)
            done += len(m)
            if s == 6 and k == 1:  # two Breaks in a row: an empty message
                assert w.write_break() == 0
                mine.append(b"")
            k += 1
        comp = w.sink
        out, pos, err = _reader_breaks(comp)
        assert err == 0 and out == b"".join(mine) and pos == list(np.cumsum([len(m) for m in mine]))
        assert resets == 3 and comp.count(b"\x80\x10\x14") >= 4
        ins.append(comp)
        msgs.append(mine)
        poss.append(pos)
    return ins, msgs, poss


def test_oracle_written_streams_split_into_their_messages(cuda, written):
    import torch

    ins, msgs, poss = written
    comp, d_coff, extent = _inputs(cuda, ins)
    idx = np.array([0] + list(np.cumsum([len(p) for p in poss])))
    pos = np.array([p for ps in poss for p in ps])
    found = len(pos)
    for max_len in CHUNK:
        got, last = _query(cuda, ins, found + 2, 0, max_len)
        assert np.array_equal(got[0], idx) and np.array_equal(got[1][:found], pos) and tuple(got[4]) == (found, found)
        assert not got[3].any() and last[0] == sum(-(-len(b) // (64 * CHUNK[max_len])) for b in ins) and last[3] > 0
    # the Python mirror, and the recipe: slots from the sizes, the decode, every stream's output split at its Breaks
    ez.select_breaks_route("p")
    try:
        brk_idx, brk_pos, sizes, status = ez.stream_breaks(comp, d_coff, in_bytes=extent)
        torch.cuda.synchronize()
        assert ez.breaks_parts_last()[0] > 0
    finally:
        ez.select_breaks_route("")
    assert np.array_equal(brk_idx.cpu().numpy(), idx) and np.array_equal(brk_pos.cpu().numpy(), pos)
    out_off = torch.zeros(len(ins) + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(sizes, 0, out=out_off[1:])
    out, sz, st = ez.decompress_batch_segmented(comp, d_coff, out_off)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and np.array_equal(sz.cpu().numpy(), sizes.cpu().numpy())
    text, off = out.cpu().numpy(), out_off.cpu().numpy()
    for s, mine in enumerate(msgs):
        cuts = [0] + pos[idx[s] : idx[s + 1]].tolist()
        assert [text[off[s] + a : off[s] + b].tobytes() for a, b in zip(cuts[:-1], cuts[1:])] == mine, s


def test_more_than_64_streams(cuda, dumped):
    e = next(e for e in dumped if e[6][256][:2] == (1, 2) and len(e[5]) >= 2 and e[1] == 0)
    group = [e] * 70
    ins = [e[2]] * 70
    want = _expected(group)
    cap = int(want[0][-1])
    got, last = _query(cuda, ins, cap)
    _assert_equals(group, got, want, cap)
    assert last[0] == 140 and last[3] == 70 * e[6][256][2], last
    wave, _ = _query(cuda, ins, cap, route="v")
    _same(got, wave, "parts against the wave route")


def test_call_order_on_left_over_scratch(cuda, dumped, written):
    import torch

    limit, group = next(_groups(dumped))
    group = [e for e in group if e[0].startswith("C256 ")][:40]
    ins = [e[2] for e in group] + written[0][:2]
    comp, d_coff, extent = _inputs(cuda, ins)
    count = len(ins)
    first, last = _query(cuda, ins, 1 << 15, limit)
    found = int(first[4][1])
    assert found > 5000 and tuple(first[4]) == (found, found) and last[0] > 0 and last[3] > 0
    side = torch.cuda.Stream(device=cuda)

    def again(what, stream=None):
        got, l = _query(cuda, ins, 1 << 15, limit, stream=stream, dirty=False)
        _same(first, got, what)
        assert l == last, (what, l)

    again("on the scratch left by itself")
    out_off = torch.zeros(count + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(torch.from_numpy(first[2]).to(cuda) + 16, 0, out=out_off[1:])
    ez.select_segments_route("p")
    try:
        ez.stream_segments(comp, d_coff, out_off, limit, seg_cap=4 * count + 64, in_bytes=extent)
        torch.cuda.synchronize()
        segs = ez.segments_parts_last()
        assert segs[0] > 0
        again("after a forced segment query")
        assert ez.segments_parts_last() == segs  # (the Break index has a scratch of its own)
    finally:
        ez.select_segments_route("")
    ez.select_size_route("p")
    try:
        ez.decompressed_sizes(comp, d_coff, limit, in_bytes=extent)
        torch.cuda.synchronize()
        assert ez.decompressed_size_parts_last()[0] > 0
        again("after a forced size query")
    finally:
        ez.select_size_route("")
    again("on a second HIP stream", side)
    again("on the first stream again")


def test_automatic_rule_is_the_wave_route(cuda, written):
    """The automatic rule ships on the wave route (breaks_parts_route: no K2b measurement stands behind
    the candidate rule yet): an unforced call with in_bytes takes no part, and gives the forced arrays."""
    ins = written[0]
    found = sum(len(p) for p in written[2])
    forced, last = _query(cuda, ins, found, 0, 1 << 20)
    auto, alast = _query(cuda, ins, found, 0, 1 << 20, route="")
    _same(forced, auto, "automatic against forced")
    assert last[0] > 0 and alast == (0, 0, 0, 0)


def test_route_entry_points(cuda):
    L = ez._lib()
    assert L.ez_select_breaks_route(ord("x")) == ez.EINVAL
    assert L.ez_select_breaks_route(ord("p")) == 0 and L.ez_select_breaks_route(ord("v")) == 0 and L.ez_select_breaks_route(0) == 0
    assert L.ez_breaks_parts_last(None) == ez.EINVAL
    c = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.ez_breaks_parts_last(c) == 0
