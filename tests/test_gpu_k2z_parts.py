"""K2z's parts route (ez_decompressed_size_batch with in_bytes: eazy_amd/csrc/ez_decompress_parts.hip,
the steps of ez_k2_parts.h), forced with ez_select_size_route('p') on hand-built streams of 2 to 7
parts, against the wave route and the oracle.

_run_parts runs a batch under a max_len hint per chunk size (256 and 1,024), with the wave route
('v') and the parts route ('p'), and checks per stream that both report (len(output), error) of the
oracle's Reader read to EOF; that the streams handed to the exact decoder (the workspace's first
words) are the same set for both, exactly the ones the test states; that the parts route reports
its chunk and as many parts walked as the streams' lengths make (so the answers are that route's,
not the wave route's behind it), the wave route none; and that nothing around out_size[0..count)
and status[0..count) is written (8 entries of -7 on both sides).  The input view lies between two
64-byte guards of 0xFF with in_off[0] != 0.  All comparisons are exact equality.  The stream
builders are tests/k2_streams.py's and tests/test_gpu_k2z.py's."""

import numpy as np
import pytest

import test_gpu_k2z as z
from k2_streams import GUARD, HDR, HDR_1K, META_BREAK, META_RESET, _forms, _oracle, assert_valid, cpy, lit, meta, rb

pytestmark = pytest.mark.gpu

LEAD = 5
EDGE = 8  # entries of -7 before and after the result arrays
HINT = {256: 4097, 1024: 1 << 20}  # a max_len hint that gives each chunk size


def _parts(ins, C):
    return sum((len(b) + 64 * C - 1) // (64 * C) for b in ins)


def _query(cuda, comp, d_coff, count, hint, route, in_bytes, limit=0, ws_init=0, keep=None):
    """One query -> (sizes, statuses, slow set, parts_last, chunk_last), the arrays' edges checked.
    ws_init: what the workspace holds when the call starts (a fill byte, or a tensor to copy from);
    it lies between two guards (tests/dirty.py), intact afterwards.  keep: a list that receives the
    workspace as the query left it."""
    import torch

    import eazy_amd as ez
    from dirty import guarded, guards_intact

    sz = torch.full((count + 2 * EDGE,), -7, dtype=torch.int64, device=cuda)
    st = torch.full((count + 2 * EDGE,), -7, dtype=torch.int32, device=cuda)
    ws_whole, ws = guarded(cuda, ez._lib().ez_decompress_workspace(count), ws_init)
    ez.select_size_route(route)
    try:
        ez.decompressed_sizes(comp, d_coff, block_size_limit=limit, sizes=sz[EDGE : EDGE + count], status=st[EDGE : EDGE + count],
                              workspace=ws, max_len=hint, in_bytes=in_bytes)
        torch.cuda.synchronize()
        last = ez.decompressed_size_parts_last()
        chunk = ez.decompressed_size_chunk_last()
    finally:
        ez.select_size_route("")
    guards_intact(ws_whole, f"route {route!r}, hint {hint}")
    if keep is not None:
        keep.append(ws.clone())
    sz, st = sz.cpu().numpy(), st.cpu().numpy()
    for a in (sz, st):
        assert (a[:EDGE] == -7).all() and (a[EDGE + count :] == -7).all(), route
    w = ws[: 4 * (count + 1)].cpu().numpy().view(np.uint32)
    slow = set(int(x) for x in w[1 : 1 + int(w[0])])
    assert int(w[0]) == len(slow)
    return sz[EDGE : EDGE + count], st[EDGE : EDGE + count], slow, last, chunk


def _upload(cuda, ins):
    import torch

    coff = LEAD + np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    ff = b"\xff" * (GUARD + LEAD)
    whole = torch.from_numpy(np.frombuffer(ff + b"".join(ins) + ff, np.uint8).copy()).to(cuda)
    comp = whole[GUARD : len(whole) - GUARD]
    assert comp.numel() == int(coff[-1]) + LEAD and coff[0] != 0
    return whole, comp, torch.from_numpy(coff).to(cuda), int(coff[-1] - coff[0])


def _want(ins, expect=None, limit=0):
    want = []
    for s, b in enumerate(ins):
        if expect and s in expect:
            want.append(expect[s])
            continue
        out, err = _oracle(b, max(1 << 20, 4 * len(b)), limit)
        if err == 2:
            out, err = _oracle(b, 1 << 26, limit)
        assert err != 2, (s, "the oracle's buffer is too small")
        want.append((len(out), err))
    return want


def _run_parts(cuda, ins, design=(), chunks=(256, 1024), expect=None, limit=0, ws_init=0, keep=None):
    """-> {C: (parts walked, taken as recorded, walked again)} of the parts route's runs.
    ws_init, keep: _query's."""
    count = len(ins)
    whole, comp, d_coff, nin = _upload(cuda, ins)
    want = _want(ins, expect, limit)
    bad = {s for s in range(count) if want[s][1] != 0} | set(design)
    got = {}
    for C in chunks:
        for route in ("v", "p"):
            sz, st, slow, last, chunk = _query(cuda, comp, d_coff, count, HINT[C], route, nin, limit, ws_init, keep)
            assert chunk == C, (C, route, chunk)
            for s in range(count):
                assert (int(sz[s]), int(st[s])) == want[s], (C, route, s, int(sz[s]), int(st[s]), want[s])
            assert slow == bad, (C, route, sorted(slow), sorted(bad))
            if route == "v":
                assert last == (0, 0, 0), last
            else:
                assert last[0] == _parts(ins, C), (C, last, _parts(ins, C))
                assert last[1] + last[2] <= last[0]
                got[C] = last
    assert np.array_equal(whole.cpu().numpy()[GUARD + LEAD : GUARD + LEAD + nin], np.frombuffer(b"".join(ins), np.uint8)), "the input was written"
    return got


def _tail3():
    return lit(b"tail!") + cpy(3, 9) + lit(b"zz")


_CACHE = {}


def _long(n, seed):
    """A valid stream of n bytes of short literals and copies."""
    if (n, seed) not in _CACHE:
        _CACHE[(n, seed)] = z.fill_to(HDR, n, np.random.default_rng(seed))
    return _CACHE[(n, seed)]


def _cuts(b):
    return [b[: len(b) - k] for k in range(1, 28)]


# ---------------------------------------------------------------- tests


@pytest.mark.parametrize("C", [256, 1024])
def test_forms_before_a_part_seam(cuda, C):
    """Every form with its first byte at each of the last 8 positions before the seam of parts 0 | 1
    (1 | 2 behind a 70,000-byte literal); 300 bytes of tokens after it."""
    rng = np.random.default_rng(307 + C)
    P = 64 * C
    far_lit = lit(rb(rng, 70000))
    lead = {}
    for far in (False, True):
        c = HDR + (far_lit if far else b"")
        at = (len(c) // P + 1) * P
        lead[far] = (z.fill_to(c, at - 300, rng), at)
    named = []
    for name, form, _, far in _forms(rng):
        for d in range(1, 9):
            c, at = lead[far]
            b = z.fill_to(c, at - d, rng) + form + _tail3()
            named.append((f"{name}-{d}", z.fill_to(b, len(b) + 300, rng)))
    assert len(named) == 21 * 8
    assert_valid(named)
    ins = [b for _, b in named]
    assert all(2 <= (len(b) + P - 1) // P <= 7 for b in ins)  # (7: the 70,000-byte forms at chunk 256)
    got = _run_parts(cuda, ins, chunks=(C,))
    assert got[C][1] > 0


@pytest.mark.parametrize("C", [256, 1024])
def test_literals_spanning_parts(cuda, C):
    """A literal from every lane of the first part that ends within a part's length, spans exactly one
    whole part, spans three whole parts: the parts it spans are passed through, neither taken nor walked."""
    rng = np.random.default_rng(311 + C)
    P = 64 * C
    body = rb(rng, 4 * P + 2000)
    ins, spanned = [], 0
    for lane in range(64):
        head = z.fill_to(HDR, lane * C + 9 + int(rng.integers(C - 9)), rng)
        for kind in range(3):
            n = P // 2 if kind == 0 else (2 * P if kind == 1 else 4 * P) - len(head) + 100 + int(rng.integers(1000))
            b = head + lit(body[:n])
            b = z.fill_to(b, (len(b) // P + 1) * P + 40, rng) + _tail3()
            assert (len(b) + P - 1) // P <= 6
            spanned += (0, 1, 3)[kind]
            ins.append(b)
    got = _run_parts(cuda, ins, chunks=(C,))
    walked, joined, again = got[C]
    assert joined > 0 and joined + again == walked - spanned, (got, spanned)


@pytest.mark.parametrize("C", [256, 1024])
def test_adversarial_and_garbage(cuda, C):
    """Literal bodies that parse as 2-byte copies on the other parity, across part seams: a part's record
    starts off the true chain and the part is walked again.  And a literal over a whole part whose body
    is wide Breaks, which the parse hands over where the chain meets one: the part's own walk meets
    them, the true chain never does, so the stream is sized and not handed over."""
    rng = np.random.default_rng(313 + C)
    P = 64 * C
    ins = []
    for parts in (2, 3):
        b = HDR + b"\x00"
        while len(b) < parts * P + 700:
            b += lit(b"\x10\x85" * 128)
        ins.append(b + _tail3())
    first_garbage = len(ins)
    for phase in range(3):
        b = z.fill_to(HDR, P // 2 + phase, rng)
        b += lit((b"\x80" + bytes([META_BREAK | 6, 0])) * (2 * P // 3))
        ins.append(z.fill_to(b, (len(b) // P + 1) * P + 40, rng) + _tail3())
    assert_valid([(str(k), b) for k, b in enumerate(ins)])
    got = _run_parts(cuda, ins, chunks=(C,))  # (the slow list is empty: no stream is handed over)
    assert got[C][1] > 0 and got[C][2] > 0, got
    # the adversarial streams alone: parts walked again
    got = _run_parts(cuda, ins[:first_garbage], chunks=(C,))
    assert got[C][2] > 0, got


@pytest.mark.parametrize("C", [256, 1024])
def test_padding_resets_and_cuts(cuda, C):
    """Padding runs of 1 to 40 bytes from 1, n/2 and n bytes before a part seam; a MetaReset after
    output in the third part (handed over by design); and one stream of each class cut at each of
    its last 27 bytes."""
    rng = np.random.default_rng(317 + C)
    P = 64 * C
    lead = z.fill_to(HDR, P - 60, rng)
    ins = []
    for n in range(1, 41):
        for d in sorted({1, (n + 1) // 2, n}):
            b = z.fill_to(lead, P - d, rng) + bytes(n) + _tail3()
            ins.append(z.fill_to(b, len(b) + 200, rng))
    reset_late = z.fill_to(z.fill_to(HDR, 2 * P + 300, rng) + meta(META_RESET, b"\x14"), 2 * P + 700, rng)
    design = [len(ins)]
    ins.append(reset_late)
    _run_parts(cuda, ins, design=design, chunks=(C,))
    big = z.fill_to(HDR, P - 20, rng) + lit(rb(rng, P + 500)) + _tail3()
    cuts = _cuts(ins[0]) + _cuts(ins[-2]) + _cuts(reset_late) + _cuts(big) + _cuts(z.fill_to(HDR, 2 * P, rng))
    want = _want(cuts)
    # (a cut may read to EOF without an error and still be handed over: a step past the input is not
    # the fast parse's to judge, tests/test_k2_size.py; the wave route's list is the reference)
    whole, comp, d_coff, nin = _upload(cuda, cuts)
    res = {r: _query(cuda, comp, d_coff, len(cuts), HINT[C], r, nin) for r in ("v", "p")}
    for r in ("v", "p"):
        sz, st, slow, last, chunk = res[r]
        assert [(int(a), int(b)) for a, b in zip(sz, st)] == want, r
        assert {s for s in range(len(cuts)) if want[s][1] != 0} <= slow
    assert res["v"][2] == res["p"][2]
    assert res["p"][3][0] == _parts(cuts, C)


def _mixed(count, rng):
    """count streams of mixed lengths: long ones of 2 to 5 parts of 16 KiB, short ones, empty ones,
    streams with errors and the forms handed over by design."""
    small = z._small_streams()
    ins, design = [], []
    for s in range(count):
        k = s % 13
        if count <= 2 or k == 0:
            ins.append(_long(33000 + 9000 * (s % 5) + s % 7, 331 + s % 4))
        elif k == 1:
            ins.append(b"")
        elif k == 2:
            ins.append(HDR)
        elif k == 3:
            ins.append(HDR + b"\x03ab")  # truncated literal
        elif k == 4:
            design.append(s)
            ins.append(HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b"))
        elif k == 5:
            ins.append(HDR_1K + lit(rb(rng, 2000)) + cpy(1500, 20) + lit(b"q"))  # distance past the window
        elif k == 6:
            ins.append(_long(20000 + s, 337)[: 17000 + s])  # a long stream cut inside a token or not
        else:
            ins.append(small[s % len(small)])
    return ins, design


@pytest.mark.parametrize("count", [1, 2, 65, 300])
def test_batches(cuda, count):
    rng = np.random.default_rng(341)
    ins, design = _mixed(count, rng)
    # (the cut long streams: handed over only if the oracle says error, which _run_parts derives)
    want = _want(ins)
    design = [s for s in design if want[s][1] == 0]
    got = _run_parts(cuda, ins, design=design, chunks=(256,))
    assert got[256][1] > 0


_MANY = {}


def many_streams(count):
    """(streams, oracle results) of a batch past kp_layout's 1,024 threads, where a thread lays out
    several streams and the last threads none: tiny valid streams of one part (the header and a short
    literal), every 97th a long one of two parts at chunk 256, every 101st empty.  Built and sized by
    the oracle once; a smaller count is a prefix."""
    if not _MANY:
        ins = []
        for s in range(2049):
            if s % 101 == 100:
                ins.append(b"")
            elif s % 97 == 96:
                ins.append(_long(17000 + s, 389))
            else:
                ins.append(HDR + lit(bytes([97 + s % 26]) * (1 + s % 5)))
        _MANY["ins"], _MANY["want"] = ins, _want(ins)
    return _MANY["ins"][:count], _MANY["want"][:count]


@pytest.mark.parametrize("count", [1025, 2049])
def test_layout_of_several_streams_per_thread(cuda, count):
    """count > 1,024: kp_layout's threads take 2 and 3 streams each and the threads past the end none
    (2,049 streams: 683 threads of 3).  Forced, chunk 256, in_bytes exact: every stream's size, status
    and place on the slow list are the oracle's, and every part was walked; in_bytes one short: the same
    results by the wave route, no part walked."""
    ins, want = many_streams(count)
    assert _parts(ins, 256) == sum(0 if not b else (2 if len(b) > 16384 else 1) for b in ins) == count - count // 101 + count // 97
    bad = {s for s in range(count) if want[s][1] != 0}
    whole, comp, d_coff, nin = _upload(cuda, ins)
    for hint in (nin, nin - 1):
        sz, st, slow, last, chunk = _query(cuda, comp, d_coff, count, HINT[256], "p", hint)
        assert chunk == 256
        got = [(int(a), int(b)) for a, b in zip(sz, st)]
        diff = [s for s in range(count) if got[s] != want[s]]
        assert not diff, (hint, diff[:4], [got[s] for s in diff[:4]], [want[s] for s in diff[:4]])
        assert slow == bad, (hint, sorted(slow)[:8], sorted(bad)[:8])
        if hint == nin:
            assert last[0] == _parts(ins, 256) and last[1] + last[2] <= last[0], last
        else:
            assert last == (0, 0, 0), last


def test_chunk_1024_batch(cuda):
    """Streams of 2 to 5 parts of 64 KiB beside short and empty ones."""
    ins = [_long(70000, 347), b"", z._small_streams()[5], _long(300000, 349), HDR, _long(131072, 353), _long(131073, 359)]
    got = _run_parts(cuda, ins, chunks=(1024,))
    assert got[1024][1] > 0


def test_bomb(cuda):
    """41-byte-class stream that claims over 10 GiB, beside long streams: 64-bit sizes on this route too."""
    bomb = HDR + lit(b"x") + cpy(1, 1 << 29) * 20
    want = 1 + 20 * (1 << 29)
    assert want > 4 << 30
    ins = [_long(40000, 331), bomb, _long(50000, 332)]
    _run_parts(cuda, ins, expect={1: (want, 0)})


def test_hints(cuda):
    """The automatic route with and without in_bytes, and the parts route under an in_bytes hint that is
    too small, exact and 4 times too large: the same results; the too-small one walks no part."""
    rng = np.random.default_rng(367)
    ins, design = _mixed(65, rng)
    want = _want(ins)
    bad = {s for s in range(len(ins)) if want[s][1] != 0} | set(design)
    whole, comp, d_coff, nin = _upload(cuda, ins)
    runs = [("", 0), ("", nin), ("p", nin - 1), ("p", nin // 2), ("p", 1), ("p", nin), ("p", 4 * nin), ("v", nin)]
    for route, hint in runs:
        sz, st, slow, last, chunk = _query(cuda, comp, d_coff, len(ins), HINT[256], route, hint)
        assert [(int(a), int(b)) for a, b in zip(sz, st)] == want, (route, hint)
        assert slow == bad, (route, hint)
        if route == "p" and hint >= nin:
            assert last[0] == _parts(ins, 256) and last[1] > 0, (route, hint, last)
        if route == "v" or hint < nin:
            assert last == (0, 0, 0), (route, hint, last)


def test_automatic_route(cuda):
    """What the library routes by itself, given in_bytes: one stream of 240 KiB or more takes the parts
    route with chunk 1,024; of two streams over 512 KiB the one that opens with a literal over half of
    it is left to the wave route by the probe and the other is cut into parts of chunk 256.  Without
    in_bytes both batches take the wave route.  The same results every way."""
    rng = np.random.default_rng(373)
    one = [_long(250000, 379)]
    two = [HDR + lit(rb(rng, 600000)) + _tail3(), _long(530000, 383)]
    for ins, hint, C, parts in ((one, 250000, 1024, 4), (two, len(two[0]), 256, (530000 + 16383) // 16384)):
        want = _want(ins)
        assert all(e == 0 for _, e in want)
        whole, comp, d_coff, nin = _upload(cuda, ins)
        for nin_hint in (nin, 0):
            sz, st, slow, last, chunk = _query(cuda, comp, d_coff, len(ins), hint, "", nin_hint)
            assert [(int(a), int(b)) for a, b in zip(sz, st)] == want and slow == set(), nin_hint
            if nin_hint:
                assert chunk == C and last[0] == parts and last[1] > 0, (chunk, last)
            else:
                assert last == (0, 0, 0), last


def test_round_trip(cuda):
    """8 x 1 MiB log-like streams: compress, query through the parts route, decode into the exact slots."""
    import torch

    import eazy_amd as ez
    from eazy_amd import synth

    count, size = 8, 1 << 20
    host = synth.logs(13, count * size)
    offs = synth.batch_offsets(count, size)
    cb = ez.compress_batch(torch.from_numpy(host).to(cuda), torch.from_numpy(offs).to(cuda), ez.MiB, 1024, max_len=size)
    packed, poff = ez.pack(cb)
    po = poff.cpu().numpy()
    nin, longest = int(po[-1] - po[0]), int((po[1:] - po[:-1]).max())
    ez.select_size_route("p")
    try:
        need, st0 = ez.decompressed_sizes(packed, poff, max_len=longest, in_bytes=nin)
        torch.cuda.synchronize()
        last = ez.decompressed_size_parts_last()
    finally:
        ez.select_size_route("")
    C = ez.decompressed_size_chunk_last()
    assert C in (256, 1024)
    assert last[0] == sum((int(n) + 64 * C - 1) // (64 * C) for n in po[1:] - po[:-1]) and last[1] > 0, last
    assert st0.cpu().numpy().tolist() == [0] * count and need.cpu().numpy().tolist() == [size] * count
    exact_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cuda), torch.cumsum(need, 0)])
    out, sizes, status = ez.decompress_batch(packed, poff, exact_off)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0] * count and sizes.cpu().numpy().tolist() == [size] * count
    assert out[: count * size].cpu().numpy().tobytes() == host.tobytes()
