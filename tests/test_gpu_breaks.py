"""K2b on the GPU: the batch Break index (ez_stream_breaks_batch), every stream's ErrBreak positions
without decoding.

The query runs on the hand-built streams of the host check (tools/k2_brk_check.hip, which writes them
with the oracle Reader's size, status and Break positions with --dump) at the three chunk sizes, on a
sub-batch view (bytes before in_off[0]), every output array and the workspace between guards, the
workspace holding 0xA5 on entry: the arrays equal the Reader's.  On the same batches out_size and
status equal ez_decompressed_size_batch's and every array equals the call without a workspace (the
exact decoder alone).  Room: brk_cap = found, found - 1 and 0 with brk_pos NULL, a batch without a
Break, count == 0, the refusals.  64 streams written by the oracle's Writer with write_break after
every message (Resets between messages, a leading Break, two in a row, one stream of about 300 KiB):
the positions are the oracle Reader's, and decompress_batch_segmented's output split at them gives
back the messages (INTEGRATION.md's recipe).  The call repeated on a workspace left by a size query,
by a decode and by itself, and on a second HIP stream, gives the same arrays.  All comparisons are
exact equality."""

import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import eazy_amd as ez
import oracle as orc
from test_k2_breaks import build_check

pytestmark = pytest.mark.gpu

PAD = 37  # bytes before in_off[0]: a sub-batch view
A5_64 = int(np.frombuffer(b"\xa5" * 8, np.int64)[0])
A5_32 = int(np.frombuffer(b"\xa5" * 4, np.int32)[0])
HINTS = {4096: 64, 1 << 16: 256, 1 << 20: 1024, 0: 256}  # max_len -> the chunk it picks


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """[(name, BlockSizeLimit, stream, size, status, [positions])] from the host check."""
    tmp = tmp_path_factory.mktemp("k2_brk_gpu")
    f = tmp / "streams.bin"
    p = subprocess.run([build_check(tmp), "--dump", str(f)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    raw, at, res = f.read_bytes(), 0, []
    while at < len(raw):
        nname, limit, nb, nbrk, size, status = struct.unpack_from("<6Q", raw, at)
        at += 48
        name = raw[at : at + nname].decode()
        at += nname
        b = raw[at : at + nb]
        at += nb
        pos = list(struct.unpack_from(f"<{nbrk}Q", raw, at))
        at += 8 * nbrk
        res.append((name, limit, b, size, status, pos))
    assert len(res) > 300 and sum(len(e[5]) for e in res) > 15000
    # (the five kinds of error in the middle and the distance over its window, each built with Breaks before it)
    assert sum(1 for e in res if e[4] != 0 and e[5]) >= 6
    return res


def _groups(dumped):
    """The dumped streams by BlockSizeLimit -> [(limit, [entries])]."""
    return [(limit, [e for e in dumped if e[1] == limit]) for limit in sorted(set(e[1] for e in dumped))]


def _guarded(cuda, n, dtype):
    """A tensor of n elements between two guards of 8 elements, everything 0xA5 bytes."""
    import torch

    whole = torch.full(((n + 16) * dtype.itemsize,), 0xA5, dtype=torch.uint8, device=cuda).view(dtype)
    return whole, whole[8 : 8 + n]


_INPUTS = {}


def _inputs(cuda, ins):
    """The batch on the device, once per list of streams -> (comp, d_coff)."""
    import torch

    key = tuple(id(b) for b in ins)  # (the streams are the fixtures' own objects: the same batch is uploaded once)
    if key not in _INPUTS:
        coff = PAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
        comp = torch.from_numpy(np.frombuffer(b"\xff" * PAD + b"".join(ins) + b"\xff" * 16, np.uint8).copy()).to(cuda)
        _INPUTS[key] = (ins, comp[: len(comp) - 16], torch.from_numpy(coff).to(cuda))
    return _INPUTS[key][1:]


def _query(cuda, ins, cap, limit=0, max_len=0, ws_init=0xA5, use_ws=True, null_pos=False, stream=None, keep=None):
    """ez_stream_breaks_batch into guarded arrays -> (brk_idx, brk_pos, sizes, status, brk_total) as
    numpy, brk_pos whole (cap entries); the guards are checked.  ws_init: what the workspace holds when
    the call starts (a fill byte, or a tensor to copy from), between its two guards (tests/dirty.py);
    use_ws False: workspace NULL; keep: a list that receives the workspace as the query left it."""
    import torch
    from dirty import guarded, guards_intact

    L = ez._lib()
    count = len(ins)
    comp, d_coff = _inputs(cuda, ins)
    arrs = [_guarded(cuda, n, dt) for n, dt in ((count + 1, torch.int64), (cap, torch.int64), (count, torch.int64), (count, torch.int32), (2, torch.int64))]
    ws_whole, ws = guarded(cuda, L.ez_breaks_workspace(count), ws_init)
    ptr = [whole.data_ptr() + 8 * whole.element_size() for whole, _ in arrs]  # (an empty view has no address of its own)
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, ptr[2], ptr[3], count, max_len, 0, 0)
    torch.cuda.synchronize()
    st = L.ez_stream_breaks_batch(limit, C.byref(b), ptr[0], None if null_pos else ptr[1], cap, ptr[4], ws.data_ptr() if use_ws else None,
                                  ez._stream_ptr(stream))
    assert st == ez.OK, st
    torch.cuda.synchronize()
    out = []
    for whole, view in arrs:
        w, a5 = whole.cpu().numpy(), A5_64 if whole.dtype == torch.int64 else A5_32
        assert (w[:8] == a5).all() and (w[-8:] == a5).all()
        out.append(view.cpu().numpy())
    guards_intact(ws_whole, "the break query")
    if not use_ws and isinstance(ws_init, int):
        assert (ws.cpu().numpy() == ws_init).all()
    if keep is not None:
        keep.append(ws.clone())
    return out


def _expected(group):
    idx = np.concatenate([[0], np.cumsum([len(e[5]) for e in group])]).astype(np.int64)
    pos = np.array([p for e in group for p in e[5]], dtype=np.int64)
    return idx, pos, np.array([e[3] for e in group], dtype=np.int64), np.array([e[4] for e in group], dtype=np.int32)


def _assert_equals(group, got, want, cap):
    """got: _query's arrays; want: _expected's; everything written, brk_pos past found untouched."""
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


@pytest.mark.parametrize("max_len", [4096, 1 << 16, 1 << 20, 0])
def test_query_equals_oracle_reader(cuda, dumped, max_len):
    assert ez._lib().ez_decompressed_size_chunk(max_len) == HINTS[max_len]
    for limit, group in _groups(dumped):
        ins = [e[2] for e in group]
        want = _expected(group)
        cap = int(want[0][-1]) + 3
        _assert_equals(group, _query(cuda, ins, cap, limit, max_len), want, cap)


def test_agrees_with_size_query_and_exact_decoder(cuda, dumped):
    import torch

    handed = 0
    for limit, group in _groups(dumped):
        ins = [e[2] for e in group]
        comp, d_coff = _inputs(cuda, ins)
        want = _expected(group)
        cap = int(want[0][-1]) + 3
        keep = []
        fast = _query(cuda, ins, cap, limit, 1 << 16, keep=keep)
        exact = _query(cuda, ins, cap, limit, 1 << 16, use_ws=False)
        for a, b in zip(fast, exact):
            assert np.array_equal(a, b)
        _assert_equals(group, exact, want, cap)
        for exact_only in (False, True):
            sz, st = ez.decompressed_sizes(comp, d_coff, limit, exact_only=exact_only, max_len=1 << 16)
            torch.cuda.synchronize()
            assert np.array_equal(sz.cpu().numpy(), fast[2]) and np.array_equal(st.cpu().numpy(), fast[3])
        # the workspace's list: the streams the walk handed to the exact decoder, and only those marked so
        w = keep[0].cpu().numpy().view(np.uint32)
        n, count = int(w[15]), len(ins)
        listed = sorted(w[16 : 16 + n].tolist())
        assert listed == np.flatnonzero(w[16 + count : 16 + 2 * count]).tolist()
        assert set(np.flatnonzero(fast[3] != 0).tolist()) <= set(listed)
        handed += n
    # (both roads ran: at least the streams built with an error go to the exact decoder, and most of the others do not)
    assert 6 <= handed < len(dumped) // 2


def test_room(cuda, dumped):
    import torch

    L = ez._lib()
    limit, group = _groups(dumped)[0]
    group = [e for e in group if len(e[2]) < 20000][:120]
    ins = [e[2] for e in group]
    want = _expected(group)
    found = int(want[0][-1])
    assert found > 100
    for use_ws in (True, False):
        _assert_equals(group, _query(cuda, ins, found, limit, use_ws=use_ws), want, found)  # brk_cap = found writes everything
        for cap, null_pos in ((found - 1, False), (0, True), (0, False)):
            brk_idx, brk_pos, sizes, status, total = _query(cuda, ins, cap, limit, use_ws=use_ws, null_pos=null_pos)
            assert tuple(total) == (0, found)
            assert np.array_equal(brk_idx, want[0]) and np.array_equal(sizes, want[2]) and np.array_equal(status, want[3])
            assert (brk_pos == A5_64).all()
    # a batch with no Break at all
    plain = [e for e in dumped if not e[5] and e[1] == limit]
    assert len(plain) >= 2
    for use_ws in (True, False):
        brk_idx, brk_pos, sizes, status, total = _query(cuda, [e[2] for e in plain], 5, limit, use_ws=use_ws)
        assert tuple(total) == (0, 0) and not brk_idx.any() and (brk_pos == A5_64).all()
        assert list(sizes) == [e[3] for e in plain] and list(status) == [e[4] for e in plain]
    # count == 0
    for use_ws in (True, False):
        brk_idx, brk_pos, sizes, status, total = _query(cuda, [], 4, use_ws=use_ws)
        assert list(brk_idx) == [0] and tuple(total) == (0, 0) and (brk_pos == A5_64).all()
    # the refusals: nothing is launched
    comp, d_coff = _inputs(cuda, ins)
    arr = torch.zeros(len(ins) + 16, dtype=torch.int64, device=cuda)
    p = arr.data_ptr()
    b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, p, None, len(ins), 0, 0, 0)
    assert L.ez_stream_breaks_batch(0, None, p, p, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), None, p, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), p, None, 4, p, None, None) == ez.EINVAL
    assert L.ez_stream_breaks_batch(0, C.byref(b), p, p, 4, None, None, None) == ez.EINVAL
    nb = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, None, None, len(ins), 0, 0, 0)
    assert L.ez_stream_breaks_batch(0, C.byref(nb), p, p, 4, p, None, None) == ez.EINVAL
    torch.cuda.synchronize()
    assert int(arr.sum()) == 0
    # the Python mirror: too little room asks again; a given brk_cap does not
    brk_idx, brk_pos, sizes, status = ez.stream_breaks(comp, d_coff, limit)
    assert np.array_equal(brk_idx.cpu().numpy(), want[0]) and np.array_equal(brk_pos.cpu().numpy(), want[1])
    assert np.array_equal(sizes.cpu().numpy(), want[2]) and np.array_equal(status.cpu().numpy(), want[3])
    brk_idx, brk_pos, _, _ = ez.stream_breaks(comp, d_coff, limit, brk_cap=found + 7)
    assert np.array_equal(brk_pos.cpu().numpy()[:found], want[1]) and int(brk_idx[-1]) == found


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
    """64 streams by the oracle's Writer, write_break after every message -> (streams, messages per
    stream as the Breaks delimit them, the Reader's positions)."""
    rng = np.random.default_rng(23)
    ins, msgs, poss = [], [], []
    for s in range(64):
        w = orc.Writer(1 << 20, 1024)
        mine = []
        if s == 5:  # starts with a Break: an empty first message
            assert w.write_break() == 0
            mine.append(b"")
        n = 300 if s == 9 else 3 + int(rng.integers(38))  # (s == 9: about 300 KiB, a Break every ~1,000 bytes)
        for k in range(n):
            if s % 4 == 1 and k and k % 3 == 0:
                w.reset()
            m = _log_lines(rng, 1000 + int(rng.integers(50)) if s == 9 else 1 + int(rng.integers(4000)))
            assert w.write(m) == (len(m), 0)
            assert w.write_break() == 0
            mine.append(m)
            if s == 6 and k == 1:  # two Breaks in a row: an empty message
                assert w.write_break() == 0
                mine.append(b"")
        comp = w.sink
        out, pos, err = _reader_breaks(comp)
        assert err == 0 and out == b"".join(mine) and len(pos) == len(mine)
        assert pos == list(np.cumsum([len(m) for m in mine]))
        ins.append(comp)
        msgs.append(mine)
        poss.append(pos)
    assert sum(len(m) for m in msgs[9]) > 290 << 10
    assert any(b"\x80\x10\x14" in b[9:] for b in ins)
    return ins, msgs, poss


def test_oracle_written_streams_split_into_their_messages(cuda, written):
    import torch

    ins, msgs, poss = written
    comp, d_coff = _inputs(cuda, ins)
    brk_idx, brk_pos, sizes, status = ez.stream_breaks(comp, d_coff, max_len=max(len(b) for b in ins))
    idx, pos = brk_idx.cpu().numpy(), brk_pos.cpu().numpy()
    assert not status.cpu().numpy().any()
    assert idx.tolist() == [0] + list(np.cumsum([len(p) for p in poss]))
    assert pos.tolist() == [p for ps in poss for p in ps]
    # the recipe: slots from the sizes, the decode, every stream's output split at its Breaks
    out_off = torch.zeros(len(ins) + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(sizes, 0, out=out_off[1:])
    out, sz, st = ez.decompress_batch_segmented(comp, d_coff, out_off)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and np.array_equal(sz.cpu().numpy(), sizes.cpu().numpy())
    text, off, sizes = out.cpu().numpy(), out_off.cpu().numpy(), sizes.cpu().numpy()
    for s, mine in enumerate(msgs):
        cuts = [0] + pos[idx[s] : idx[s + 1]].tolist()
        got = [text[off[s] + a : off[s] + b].tobytes() for a, b in zip(cuts[:-1], cuts[1:])]
        assert got == mine, s
        assert cuts[-1] == sizes[s]  # (every message here ends in a Break)
    # the same arrays from the guarded call at every chunk size and from the exact decoder alone
    found = len(pos)
    for max_len, use_ws in ((4096, True), (1 << 16, True), (1 << 20, True), (0, False)):
        g = _query(cuda, ins, found + 2, 0, max_len, use_ws=use_ws)
        assert np.array_equal(g[0], idx) and np.array_equal(g[1][:found], pos) and tuple(g[4]) == (found, found)


def test_dirty_workspace_and_call_order(cuda, dumped, written):
    import torch

    limit, group = _groups(dumped)[0]
    group = [e for e in group if len(e[2]) < 20000][:150]
    ins = [e[2] for e in group] + written[0][:8]
    comp, d_coff = _inputs(cuda, ins)
    count = len(ins)
    first = _query(cuda, ins, 1 << 15, limit, ws_init=0)
    found = int(first[4][1])
    assert found > 100 and tuple(first[4]) == (found, found)
    L = ez._lib()
    # left by a size query and by a decode (their workspace is larger: its first bytes are what this one starts with)
    big = torch.full((L.ez_decompress_workspace(count),), 0x5A, dtype=torch.uint8, device=cuda)
    ez.decompressed_sizes(comp, d_coff, limit, workspace=big)
    torch.cuda.synchronize()
    after_size = big.clone()
    out_off = torch.zeros(count + 1, dtype=torch.int64, device=cuda)
    torch.cumsum(torch.from_numpy(first[2]).to(cuda) + 16, 0, out=out_off[1:])
    ez.decompress_batch(comp, d_coff, out_off, limit, workspace=big)
    torch.cuda.synchronize()
    after_decode = big.clone()
    keep = []
    _query(cuda, ins[: count // 2] + ins[: count - count // 2], 1 << 15, limit, keep=keep)  # left by itself, on another batch of the same count
    side = torch.cuda.Stream(device=cuda)
    for ws_init, stream in ((after_size, None), (after_decode, None), (keep[0], None), (0xFF, None), (keep[0], side), (0x00, side)):
        again = _query(cuda, ins, 1 << 15, limit, ws_init=ws_init, stream=stream)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
