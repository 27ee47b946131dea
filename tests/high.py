"""Where a batch lies: the hand-built groups of the route tests placed high in buffers of more than
4 GiB, and runners that hold those tests' bars there (tests/test_gpu_high_offsets.py).

ez_batch's offsets are absolute and 64-bit; inside the kernels nearly every position is 32-bit.  The
route tests put every batch at offset 0 of a buffer of a few MiB, so an offset truncated to 32 bits
or sign-extended from 31 would pass them.  Here the base pointers are those of three buffers of SPAN
bytes (Big) and the batch's first offsets are a placement's (in_base, out_base):

  in-straddles-2^32    (2^32 - h_in, 3)             2^32 falls inside the input
  out-straddles-2^32   (5, 2^32 - h_out)            2^32 falls inside the output slots
  both-above-2^32      (2^32 + 5, 2^32 + 9)         everything above, unaligned
  both-straddle-2^31   (2^31 - h_in, 2^31 - h_out)  2^31 falls inside both (sign extension)

h: half the batch's bytes on that side, made odd.  The buffers are real allocations over their whole
length: IN holds 0x5A, SLOTS and OUT hold FILL.  A store through a truncated offset lands 2^32 or 2^31
below its target inside the same buffer, where Big.verify finds it (every byte outside the batch's
own slots is checked after every call, in chunks on the device); a load through one reads 0x5A or
another stream and fails the oracle comparison.

The runners restate the bars of test_gpu_k1_edges.run_route, k2_streams._run and the query tests'
_query / _decode_both for a placed batch; what they compare against (the oracle's bytes, the Reader's
sizes and statuses, the host walks' arrays) is computed as those tests compute it."""

import numpy as np

MiB, GiB = 1 << 20, 1 << 30
SPAN = (1 << 32) + (64 << 20)  # bytes of each of the three buffers
IN_FILL, FILL = 0x5A, 0xA5  # FILL: the K1 and K2 runners' sentinel
T32, T31 = 1 << 32, 1 << 31

PLACEMENTS = ("in-straddles-2^32", "out-straddles-2^32", "both-above-2^32", "both-straddle-2^31")
# the power of two a placement puts inside the batch's input / output (None: the side lies low, or wholly above 2^32)
INSIDE = {PLACEMENTS[0]: (T32, None), PLACEMENTS[1]: (None, T32), PLACEMENTS[2]: (None, None), PLACEMENTS[3]: (T31, T31)}


def odd_half(n):
    return (int(n) // 2) | 1


def place(p, in_bytes, out_bytes):
    """(in_base, out_base) of placement p for a batch of in_bytes of input and out_bytes of slots."""
    h_in, h_out = odd_half(in_bytes), odd_half(out_bytes)
    return {PLACEMENTS[0]: (T32 - h_in, 3), PLACEMENTS[1]: (5, T32 - h_out), PLACEMENTS[2]: (T32 + 5, T32 + 9),
            PLACEMENTS[3]: (T31 - h_in, T31 - h_out)}[p]


def offsets(base, lens):
    return (int(base) + np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])).astype(np.int64)


def claims(p, in_off, out_off):
    """Arithmetic on the offsets alone: -> (the batch is placed as p says, the named power of two falls
    strictly inside a stream's input or slot).  A power that coincides with an offset (in_off[0] above
    all) is inside nothing."""
    batch, stream = True, False
    for t, off in zip(INSIDE[p], (in_off, out_off)):
        if t is None:
            continue
        batch = batch and bool(off[0] < t < off[-1])
        stream = stream or bool(((off[:-1] < t) & (t < off[1:])).any())
    if p == PLACEMENTS[2]:
        batch = bool(in_off[0] > T32 and out_off[0] > T32 and in_off[0] % 16 and out_off[0] % 16)
    if p == PLACEMENTS[0]:
        batch = batch and out_off[-1] < T31
    if p == PLACEMENTS[1]:
        batch = batch and in_off[-1] < T31
    return batch and int(out_off[-1]) <= SPAN and int(in_off[-1]) <= SPAN, stream


# ------------------------------------------------------------------ the three buffers

_CHUNK = 1 << 25  # int64 words compared at a time: 256 MiB read, a 32 MiB temporary


def _pattern(byte):
    return int(np.frombuffer(bytes([byte]) * 8, np.int64)[0])


def strays(buf, byte, allowed):
    """The first few positions of buf outside the intervals `allowed` ([(a, b)], any order, may
    overlap) whose byte is not `byte` ([]: none).  Long gaps are compared eight bytes at a time in
    chunks on the device, the short ones gathered into one tensor."""
    import torch

    n, at, gaps = buf.numel(), 0, []
    for a, b in sorted((max(0, int(a)), min(int(b), buf.numel())) for a, b in allowed):
        if a > at:
            gaps.append((at, a))
        at = max(at, b)
    if at < n:
        gaps.append((at, n))
    words, pat = buf[: n // 8 * 8].view(torch.int64), _pattern(byte)
    bad = torch.zeros((), dtype=torch.bool, device=buf.device)
    short, long = [], []
    for a, b in gaps:
        a8, b8 = -(-a // 8) * 8, b // 8 * 8
        if b8 - a8 < 4096:
            short.append((a, b))
            continue
        short += [(a, a8), (b8, b)]
        for k in range(a8 // 8, b8 // 8, _CHUNK):
            long.append((k, min(k + _CHUNK, b8 // 8)))
            bad |= (words[long[-1][0] : long[-1][1]] != pat).any()
    short = [(a, b) for a, b in short if b > a]
    if short:
        bad |= (torch.cat([buf[a:b] for a, b in short]) != byte).any()
    if not bool(bad):
        return []
    found = []
    for a, b in short:
        found += [a + int(k) for k in torch.nonzero(buf[a:b] != byte)[:8, 0]]
    for k0, k1 in long:
        w = torch.nonzero(words[k0:k1] != pat)[:8, 0]
        for k in w.tolist():
            q = 8 * (k0 + k)
            found += [q + int(j) for j in torch.nonzero(buf[q : q + 8] != byte)[:, 0]]
    return sorted(found)[:8]


WANT_GIB = {"A": 16, "B": 16, "B-K2j": 40, "C": 48}


def want_memory(part):
    """pytest.skip unless WANT_GIB[part] GiB of device memory are free (with the library's cached
    scratch released first), test_p4_offsets_past_4gib's rule."""
    import pytest
    import torch

    import eazy_amd as ez

    ez.release_cached()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < WANT_GIB[part] << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free, part {part} wants {WANT_GIB[part]}")


class Big:
    """IN (0x5A), SLOTS and OUT (FILL), SPAN bytes each."""

    def __init__(self, cuda):
        import torch

        self.cuda = cuda
        self.IN = torch.full((SPAN,), IN_FILL, dtype=torch.uint8, device=cuda)
        self.SLOTS = torch.full((SPAN,), FILL, dtype=torch.uint8, device=cuda)
        self.OUT = torch.full((SPAN,), FILL, dtype=torch.uint8, device=cuda)
        self.held = None  # (where the input lies, its bytes)

    def put(self, data, at):
        """The batch's input at IN[at:]."""
        import torch

        host = np.frombuffer(data, np.uint8).copy() if isinstance(data, (bytes, bytearray)) else np.array(data, dtype=np.uint8)
        assert 0 <= at and at + len(host) <= SPAN
        self.IN[at : at + len(host)].copy_(torch.from_numpy(host).to(self.cuda))
        self.held = (int(at), host)

    def clear(self, slots=(), out=()):
        """IN back to 0x5A; the given intervals of SLOTS and OUT back to FILL."""
        if self.held is not None:
            at, host = self.held
            self.IN[at : at + len(host)].fill_(IN_FILL)
            self.held = None
        for buf, spans in ((self.SLOTS, slots), (self.OUT, out)):
            for a, b in spans:
                buf[int(a) : int(b)].fill_(FILL)

    def verify(self, what, slots=(), out=(), owners=()):
        """After a call: IN is unchanged over its whole length; every byte of SLOTS and OUT outside the
        intervals given (what the call may have written) is FILL.  owners: [(a, b, name)], the streams'
        slots: a stray byte 2^32 or 2^31 below one of them is reported with that stream's name.  On a
        failure the buffers are made whole again, so that the next case starts clean."""
        import torch

        at, host = self.held if self.held is not None else (0, np.zeros(0, np.uint8))
        msgs = []
        got = self.IN[at : at + len(host)].cpu().numpy()
        if not np.array_equal(got, host):
            k = int(np.flatnonzero(got != host)[0])
            msgs.append(f"the input was written: byte {k} of the batch (IN[{at + k}]) is {got[k]:#04x}")
        for name, buf, byte, allowed in (("IN", self.IN, IN_FILL, [(at, at + len(host))]), ("SLOTS", self.SLOTS, FILL, slots), ("OUT", self.OUT, FILL, out)):
            bad = strays(buf, byte, allowed)
            if bad:
                ext = [(int(a), int(b)) for a, b in allowed]
                lo, hi = (min(a for a, _ in ext), max(b for _, b in ext)) if ext else (None, None)
                vals = [int(buf[k]) for k in bad[:4]]
                for d, dn in ((T32, "2^32"), (T31, "2^31")):
                    own = [nm for a, b, nm in owners if a <= bad[0] + d < b]
                    if own:
                        msgs.append(f"the first stray byte lies {dn} below the slot of {own[0]}")
                msgs.append(f"{name} written outside the batch's own bytes at {bad} (values {vals}; the batch's lie in [{lo}, {hi}): "
                            f"{[k - lo for k in bad] if ext else ''} from its start, 2^32 below is {[k + T32 - lo for k in bad[:2]] if ext else ''})")
                buf.fill_(byte)
                if name == "IN":
                    self.IN[at : at + len(host)].copy_(torch.from_numpy(host).to(self.cuda))
        assert not msgs, f"{what}: " + "; ".join(msgs)


# ------------------------------------------------------------------ K1 (test_gpu_k1_edges.run_route's bar)


def k1_layout(p, bufs, want):
    """-> (in_off, slot_off) of the batch at placement p: the slots are exactly the oracle's lengths, back to back."""
    in_base, out_base = place(p, sum(len(b) for b in bufs), sum(len(w) for w in want))
    return offsets(in_base, [len(b) for b in bufs]), offsets(out_base, [len(w) for w in want])


def run_k1(big, p, what, named, block, htable, kind, max_len, route):
    """One batch on one route at placement p, held to run_route's bar: the route's name; status 0, the
    oracle's size and bytes for every stream in a slot of exactly that size, the slots back to back;
    everything else in SLOTS, OUT and IN unchanged; the packed batch decodes back to the input on the
    automatic K2, into OUT at the placement's output base."""
    import torch

    import eazy_amd as ez
    from test_gpu_k1_edges import first_difference, oracle_bytes

    cuda = big.cuda
    names = [n for n, _ in named]
    bufs = [b for _, b in named]
    count = len(bufs)
    want = [oracle_bytes(b, block, htable) for b in bufs]
    in_off, so = k1_layout(p, bufs, want)
    ok, _ = claims(p, in_off, so)
    assert ok, (p, in_off[[0, -1]], so[[0, -1]])
    host = np.frombuffer(b"".join(bufs), np.uint8)
    big.put(host, int(in_off[0]))
    d_in_off, d_so = torch.from_numpy(in_off).to(cuda), torch.from_numpy(so).to(cuda)
    cb = ez.CompressedBatch(big.SLOTS, d_so, torch.full((count,), -1, dtype=torch.int64, device=cuda),
                            torch.full((count,), -1, dtype=torch.int32, device=cuda))
    written, decoded = [(so[0], so[-1])], []
    try:
        ez.select_compress_kernel(kind)
        try:
            ez.compress_batch(big.IN, d_in_off, block, htable, max_len=max_len, out=cb)
            torch.cuda.synchronize()
            got_route = ez.compress_route_last()
        finally:
            ez.select_compress_kernel("")
        what = f"{what} at {p} (in_off[0] {in_off[0]}, out_off[0] {so[0]}) on {got_route!r} (kind {kind!r}, max_len {max_len}, block {block}, htable {htable})"
        assert got_route == route, f"{what}: expected route {route!r}"
        st, sz = cb.status.cpu().numpy(), cb.sizes.cpu().numpy()
        slots = big.SLOTS[int(so[0]) : int(so[-1])].cpu().numpy()
        bad = []
        for s, w in enumerate(want):
            o = int(so[s] - so[0])
            got = slots[o : o + max(int(sz[s]), 0)].tobytes()
            if st[s] != 0 or got != w:
                bad.append(f"{names[s]} (stream {s}, {len(bufs[s])} bytes at in_off {in_off[s]}, slot at {so[s]}): status {st[s]}, {sz[s]} bytes, "
                           f"the oracle {len(w)}; {first_difference(got, w)}")
        big.verify(what, slots=written, owners=[(so[s], so[s + 1], f"{names[s]} (stream {s})") for s in range(count)])
        assert not bad, f"{what}: {len(bad)} of {len(want)} streams differ from the oracle:\n" + "\n".join(bad[:12])
        # the packed batch (K3 reads the slots at their high offsets) decodes back to the input
        packed = torch.empty(int(so[-1] - so[0]) + 16, dtype=torch.uint8, device=cuda)
        poff = torch.empty(count + 1, dtype=torch.int64, device=cuda)
        ez.pack(cb, packed, poff)
        torch.cuda.synchronize()
        assert np.array_equal(poff.cpu().numpy(), so - so[0]), f"{what}: packed_off is not the sizes' cumsum"
        ooff = offsets(place(p, len(host), len(host))[1], [len(b) for b in bufs])
        decoded = [(ooff[0], ooff[-1])]
        _, dsz, dst = ez.decompress_batch(packed, poff, torch.from_numpy(ooff).to(cuda), out=big.OUT)
        torch.cuda.synchronize()
        assert int(dst.abs().sum()) == 0 and dsz.cpu().tolist() == [len(b) for b in bufs], f"{what}: decode"
        assert big.OUT[int(ooff[0]) : int(ooff[-1])].cpu().numpy().tobytes() == host.tobytes(), f"{what}: the decoded bytes are not the input"
        big.verify(what + ", packed and decoded", slots=written, out=decoded)
    finally:
        big.clear(slots=written, out=decoded)
    return got_route


# ------------------------------------------------------------------ K2 (k2_streams._run's bar)


def k2_layout(p, ins, slots=None, lim=0):
    """-> (comp_off, out_off, cap) of the batch at placement p, with _run's slots (the oracle's length
    plus 1..5 bytes, never a multiple of 16) unless `slots` ({index: bytes}) says otherwise."""
    from k2_streams import _need, _slot

    cap = [slots[s] if slots and s in slots else _slot(s, _need(b, lim)) for s, b in enumerate(ins)]
    in_base, out_base = place(p, sum(len(b) for b in ins), sum(cap))
    return offsets(in_base, [len(b) for b in ins]), offsets(out_base, cap), cap


def _fetch(buf, spans):
    """The bytes of buf in every [a, b) of spans, through one transfer -> [bytes]."""
    import torch

    spans = [(int(a), int(b)) for a, b in spans]
    flat = torch.cat([buf[a:b] for a, b in spans]).cpu().numpy() if spans else np.zeros(0, np.uint8)
    at, res = 0, []
    for a, b in spans:
        res.append(flat[at : at + b - a].tobytes())
        at += b - a
    return res


def run_k2(big, p, ins, jc=None, slots=None, handed="auto", kind="j", max_len=None, hints=None, layout=None, what=""):
    """Decode ins at placement p with the decoder `kind` forced ("j", "r", "t", "w"; "exact": the exact
    decoder alone, exact_only=True) and hold _run's bar: status, size and bytes of every stream equal
    the oracle's and the exact decoder's (run behind the forced one on the same placement); every byte of
    OUT outside [out_off[s], out_off[s] + size) keeps FILL (the slot slack included; for a stream that
    ends in an error only the bytes outside its slot), over the buffer's whole length; IN and SLOTS are
    unchanged; the streams handed to the exact decoder (the workspace's first words) are exactly the
    ones expected; the decoder that ran is the one forced.  The workspace lies between the guards of
    tests/dirty.py and holds 0xA5 on entry.  layout: (comp_off, out_off, cap) instead of k2_layout's.
    hints: f(in_bytes, out_bytes) -> kwargs.  -> the streams handed over."""
    import torch

    import eazy_amd as ez
    from dirty import guarded, guards_intact
    from k2_streams import SMALL_MAX, _oracle

    cuda = big.cuda
    count = len(ins)
    total_in = sum(len(b) for b in ins)
    if kind == "j":
        assert (256 if total_in <= SMALL_MAX else 1024) == jc, (total_in, jc)
    coff, ooff, cap = layout if layout is not None else k2_layout(p, ins, slots)
    if layout is None:
        ok, _ = claims(p, coff, ooff)
        assert ok, (p, coff[[0, -1]], ooff[[0, -1]])
    what = f"{what} K2{kind} at {p} (in_off[0] {coff[0]}, out_off[0] {ooff[0]})"
    big.put(b"".join(ins), int(coff[0]))
    d_coff, d_ooff = torch.from_numpy(coff).to(cuda), torch.from_numpy(ooff).to(cuda)
    kw = hints(int(coff[-1] - coff[0]), int(ooff[-1] - ooff[0])) if hints else {}
    if max_len is not None:
        kw["max_len"] = max(cap) if max_len is True else max_len
    res = []
    try:
        for exact in (False, True) if kind != "exact" else (True,):
            sz = torch.full((count,), -7, dtype=torch.int64, device=cuda)
            st = torch.full((count,), -7, dtype=torch.int32, device=cuda)
            ws_whole, ws = guarded(cuda, ez._lib().ez_decompress_workspace(count), 0xA5)
            ws0 = ws.clone()
            ez.select_decompress_kernel("" if exact else kind)
            try:
                ez.decompress_batch(big.IN, d_coff, d_ooff, out=big.OUT, sizes=sz, status=st, workspace=ws, exact_only=exact, **kw)
                torch.cuda.synchronize()
                took = ez.decompress_kernel_last()
            finally:
                ez.select_decompress_kernel("")
            who = "the exact decoder" if exact else "K2" + kind
            guards_intact(ws_whole, who)
            if exact:
                assert took == "e", took
                assert torch.equal(ws, ws0), "the exact decoder alone wrote the workspace"
            else:
                assert took == kind, f"{what}: the batch took {took!r}"
            h_sz, h_st = sz.cpu().numpy(), st.cpu().numpy()
            assert ((0 <= h_sz) & (h_sz <= np.asarray(cap))).all(), (who, h_sz, cap)
            # (K2r and K2t may have written part of a slot before they hand a stream with an error over)
            may = [(ooff[s], ooff[s] + (h_sz[s] if h_st[s] == 0 or kind == "j" else cap[s])) for s in range(count)]
            try:
                big.verify(f"{what}, {who}", out=may, owners=[(ooff[s], ooff[s + 1], f"stream {s}") for s in range(count)])
                data = _fetch(big.OUT, [(ooff[s], ooff[s] + h_sz[s]) for s in range(count)])
            finally:
                for a, b in may:
                    big.OUT[int(a) : int(b)].fill_(FILL)
            res.append((data, h_sz, h_st, ws[: 4 * (count + 1)].cpu().numpy().view(np.uint32)))
    finally:
        big.clear()
    (out, sz, st, w), (xout, xsz, xst, _) = res[0], res[-1]
    bad = set()
    for s, b in enumerate(ins):
        want, err = _oracle(b, cap[s], 0)
        assert st[s] == xst[s] and sz[s] == xsz[s], (what, s, st[s], xst[s], sz[s], xsz[s])
        assert out[s] == xout[s], f"{what}: stream {s} (slot at {ooff[s]}) differs from the exact decoder's"
        if err == 2:  # the oracle's output exceeded the slot
            assert st[s] == ez.ENOSPC, (what, s, st[s])
            bad.add(s)
            continue
        assert st[s] == err, (what, s, st[s], err)
        assert int(sz[s]) == len(want), (what, s, sz[s], len(want))
        assert out[s] == want, f"{what}: stream {s} (slot at {ooff[s]}, input at {coff[s]}) differs from the oracle's"
        if err != 0:
            bad.add(s)
    got = set(int(x) for x in w[1 : 1 + min(int(w[0]), count)])
    if handed is not None and kind != "exact":
        assert int(w[0]) == len(got), (what, int(w[0]), sorted(got))
        expect = bad if handed == "auto" else (set(range(count)) if handed == "all" else set(handed))
        assert got == expect, f"{what}: handed over {sorted(got)}, expected {sorted(expect)}"
    return got


# ------------------------------------------------------------------ the segmented decode (test_gpu_segments._decode_both's bar)


def run_segmented(big, p, ins, caps, route, what=""):
    """decompress_batch_segmented at placement p under the segment query's route ('v' wave, 'p' parts)
    against the oracle and the exact decoder on the same placement: equal sizes, statuses and bytes,
    FILL intact outside every slot and in the slack of the streams that end OK, the OK streams' bytes
    the oracle's.  -> (sizes, statuses, segments_last(), segments_parts_last())."""
    import torch

    import eazy_amd as ez
    from k2_streams import _oracle

    cuda = big.cuda
    count = len(ins)
    in_base, out_base = place(p, sum(len(b) for b in ins), sum(caps))
    coff, ooff = offsets(in_base, [len(b) for b in ins]), offsets(out_base, caps)
    ok, _ = claims(p, coff, ooff)
    assert ok, (p, coff[[0, -1]], ooff[[0, -1]])
    what = f"{what} segmented decode, route {route!r}, at {p} (in_off[0] {coff[0]}, out_off[0] {ooff[0]})"
    big.put(b"".join(ins), int(coff[0]))
    d_coff, d_ooff = torch.from_numpy(coff).to(cuda), torch.from_numpy(ooff).to(cuda)
    res = []
    try:
        for exact in (False, True):
            sz = torch.full((count,), -7, dtype=torch.int64, device=cuda)
            st = torch.full((count,), -7, dtype=torch.int32, device=cuda)
            if exact:
                ez.decompress_batch(big.IN, d_coff, d_ooff, out=big.OUT, sizes=sz, status=st, exact_only=True)
                torch.cuda.synchronize()
            else:
                ez.select_segments_route(route)
                try:
                    ez.decompress_batch_segmented(big.IN, d_coff, d_ooff, out=big.OUT, sizes=sz, status=st, in_bytes=int(coff[-1] - coff[0]))
                    torch.cuda.synchronize()
                    segs, parts = ez.segments_last(), ez.segments_parts_last()
                finally:
                    ez.select_segments_route("")
            h_sz, h_st = sz.cpu().numpy(), st.cpu().numpy()
            assert ((0 <= h_sz) & (h_sz <= np.asarray(caps))).all(), (what, h_sz, caps)
            may = [(ooff[s], ooff[s] + (h_sz[s] if h_st[s] == 0 else caps[s])) for s in range(count)]
            try:
                big.verify(f"{what}, {'the exact decoder' if exact else 'segmented'}", out=may)
                data = _fetch(big.OUT, [(ooff[s], ooff[s] + h_sz[s]) for s in range(count)])
            finally:
                for a, b in may:
                    big.OUT[int(a) : int(b)].fill_(FILL)
            res.append((data, h_sz, h_st))
    finally:
        big.clear()
    (out, sz, st), (xout, xsz, xst) = res
    bad = np.flatnonzero((sz != xsz) | (st != xst))
    assert bad.size == 0, (what, bad[:4], sz[bad[:4]], xsz[bad[:4]], st[bad[:4]], xst[bad[:4]])
    for s, b in enumerate(ins):
        assert out[s] == xout[s], f"{what}: stream {s} differs from the exact decoder's"
        want, err = _oracle(b, caps[s], 0)
        if err == 2:
            assert st[s] == ez.ENOSPC, (what, s, st[s])
            continue
        assert (st[s], int(sz[s])) == (err, len(want)), (what, s, st[s], err, sz[s], len(want))
        if err == 0:
            assert out[s] == want, f"{what}: stream {s} (slot at {ooff[s]}, input at {coff[s]}) differs from the oracle's"
    return sz, st, segs, parts


# ------------------------------------------------------------------ the pure queries


class Query:
    """A batch of compressed streams at a placement's input base (the out_off a query takes only
    enters its arithmetic; it gets the placement's output base all the same)."""

    def __init__(self, big, p, ins, caps=None):
        import torch

        self.big, self.p, self.count = big, p, len(ins)
        caps = [1] * len(ins) if caps is None else caps
        in_base, out_base = place(p, sum(len(b) for b in ins), sum(caps))
        self.coff, self.ooff = offsets(in_base, [len(b) for b in ins]), offsets(out_base, caps)
        t = INSIDE[p][0]
        assert in_base > T32 if t is None else self.coff[0] < t < self.coff[-1], (p, self.coff[[0, -1]])
        self.in_bytes = int(self.coff[-1] - self.coff[0])
        big.put(b"".join(ins), in_base)
        self.d_coff, self.d_ooff = torch.from_numpy(self.coff).to(big.cuda), torch.from_numpy(self.ooff).to(big.cuda)

    def done(self, what):
        """No query writes any of the three buffers."""
        try:
            self.big.verify(f"{what} at {self.p} (in_off[0] {self.coff[0]})")
        finally:
            self.big.clear()


def ws_for(cuda, nbytes):
    from dirty import guarded

    return guarded(cuda, nbytes, 0xA5)
