"""The compress-side hints (ez_batch.max_len, max_writes) on every K1 route.

INTEGRATION.md §4: max_len sizes a route's scratch and picks the route; a larger hint
changes nothing else, a stream of exactly max_len bytes is accepted, a longer one is
refused (EZ_EINVAL, size 0, nothing in its slot) and its neighbours are untouched;
0 = unknown takes the general kernel.  Every call below names the route it means to
reach and checks it with ez_compress_route_last.

Bar: byte-exact against the oracle, stream by stream.  The oracle's result of a batch
is computed once and shared by every hint.

The GPU tests are marked one by one (not with a module mark): the first test checks on
the CPU that the shared inputs contain what they claim."""

import functools

import numpy as np
import pytest

import oracle as orc

MiB = 1 << 20
GUARD = 64  # sentinel bytes before the first slot and after the last
FILL = 0xA5


# ------------------------------------------------------------------ inputs


def _log_planted(seed, n):
    """n bytes of logs with copies planted: earlier stretches (near and far), short-period
    runs and zero runs, about one per 600 bytes."""
    from eazy_amd import synth

    rng = np.random.default_rng(seed)
    b = bytearray(synth.logs(seed, n).tobytes())
    for p in np.sort(rng.integers(64, max(65, n - 64), max(2, n // 600))):
        p = int(p)
        L = int(rng.integers(6, 48))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            d = int(rng.integers(1, p))
            for t in range(min(L, n - p)):
                b[p + t] = b[p - d + t]
        elif kind == 1:
            per = int(rng.integers(1, 9))
            for t in range(per, min(L, n - p)):
                b[p + t] = b[p + t - per]
        else:
            b[p : p + L] = bytes(min(L, n - p))
    return bytes(b[:n])


@functools.lru_cache(maxsize=None)
def hint_streams():
    """About 40 streams of at most 4096 bytes (one of exactly 4096): the hand-picked tiny ones,
    random bytes with planted window matches, runs and zero runs, ragged log slices.  The first
    and the last are live (>= 4 bytes) and shorter than 16 bytes: k1_lean's edge-slot path."""
    from eazy_amd import synth
    from test_gpu_batch import _planted

    rng = np.random.default_rng(101)
    d = synth.logs(103, 1 << 18).tobytes()
    bufs = [b"abcdeabcde"]
    at = 0
    for n in (0, 1, 3, 4, 5, 17):
        bufs.append(d[at : at + n])
        at += n
    bufs.append(b"abcdefg" * 41)  # a 7-byte period
    for z in (7, 8, 9):  # zero runs around writeZeros's 8-byte test
        bufs.append(b"head" + bytes(z) + b"tail-of-the-stream" + bytes(z) + b"x")
    bufs += [_planted(rng, n, e, 4096, zeros=True) for n, e in ((4096, 40), (3001, 25), (1500, 12), (700, 6))]
    bufs.append(bytes(300) + d[at : at + 500] + bytes(1000))
    lens = [4096, 4095, 4093, 17, 33] + [int(v) for v in rng.integers(20, 4096, 17)]
    for n in lens:
        bufs.append(d[at : at + n])
        at += n
    bufs.append(_log_planted(107, 2500))
    bufs.append(b"0123456789ab")
    assert max(len(b) for b in bufs) == 4096 and 4 <= len(bufs[0]) < 16 and 4 <= len(bufs[-1]) < 16
    return tuple(bufs)


@functools.lru_cache(maxsize=None)
def big_streams():
    """4 x 256 KiB of logs (the decode hint's second batch)."""
    from eazy_amd import synth

    d = synth.logs(109, 4 << 18).tobytes()
    return tuple(d[k << 18 : (k + 1) << 18] for k in range(4))


_ORACLE = {}


def oracle_of(bufs, htable=1024, magic=True, block=MiB):
    """The oracle's streams of a batch of single Writes (tuple of bytes), computed once."""
    key = (bufs, htable, magic, block)
    if key not in _ORACLE:
        _ORACLE[key] = [orc.compress(block, htable, [b], append_magic=magic) for b in bufs]
    return _ORACLE[key]


def token_census(comp: bytes):
    """Counts of the stream's tokens, walked with eazy_amd.dump: literals, copies, zero-run
    copies (OffLong, 0), and copies by the bytes of their offset field."""
    import eazy_amd as ez

    seen = {"l": 0, "c": 0, "z": 0, 1: 0, 2: 0, 3: 0}
    dec = ez.Decoder()

    def dbg(ioff, iend, ooff, tag, l, off):
        if tag == ord("l"):
            seen["l"] += 1
        elif tag == ord("c"):
            seen["c"] += 1
            _, _, i2, e = dec.tag(comp, ioff)
            assert e == 0
            field = comp[i2:iend]
            if field == bytes([ez.OffLong, 0]):
                seen["z"] += 1
            elif len(field) in seen:
                seen[len(field)] += 1

    dmp = ez.NewDumper()
    dmp.Debug = dbg
    n, err = dmp.Write(comp)
    assert err == 0 and n == len(comp)
    return seen


def test_hint_inputs_contain_their_forms():
    """CPU: over the shared streams the oracle emits literals, copies, zero-run tokens and
    offsets in the one-, two- and three-byte forms, and every stream of 600 bytes or more holds
    copies and literals -- so the GPU
    tests below cannot pass on inputs that parse to one literal each."""
    total = {"l": 0, "c": 0, "z": 0, 1: 0, 2: 0, 3: 0}
    for b, comp in zip(hint_streams(), oracle_of(hint_streams())):
        c = token_census(comp)
        for k in total:
            total[k] += c[k]
        assert len(b) < 600 or (c["c"] > 0 and c["l"] > 0), f"a stream of {len(b)} bytes without a copy or a literal"
    assert all(total[k] > 0 for k in total), total
    assert total["z"] >= 4, total  # the planted zero runs, and the 8- and 9-byte ones
    # the boundary streams of C2 / C3 and the multi-Write batch hold copies too
    assert token_census(orc.compress(MiB, 1024, [_log_planted(4096, 4096)]))["c"] > 5
    for ws in multi_write_streams():
        if sum(len(w) for w in ws) > 600:
            assert token_census(orc.compress(MiB, 1024, list(ws)))["c"] > 0


# ------------------------------------------------------------------ device helpers


class DevBatch:
    """A batch's bytes and offsets on the device, uploaded once."""

    def __init__(self, cuda, bufs):
        import torch

        self.bufs = bufs
        self.lens = np.array([len(b) for b in bufs], np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.host = np.frombuffer(b"".join(bufs), np.uint8).copy()
        self.data = torch.from_numpy(self.host).to(cuda)
        self.off = torch.from_numpy(self.offs).to(cuda)
        self.cuda = cuda

    def guarded(self, slot_off=None):
        """A CompressedBatch filled with FILL whose slots start GUARD bytes into the buffer
        (offsets are absolute) and end GUARD bytes before its end."""
        import torch

        import eazy_amd as ez

        so = (ez.slot_offsets(self.off) if slot_off is None else slot_off) + GUARD
        total = int(so[-1].item()) + GUARD
        n = len(self.bufs)
        return ez.CompressedBatch(
            torch.full((total,), FILL, dtype=torch.uint8, device=self.cuda),
            so,
            torch.full((n,), -1, dtype=torch.int64, device=self.cuda),
            torch.full((n,), -1, dtype=torch.int32, device=self.cuda),
        )


def run_k1(dev, max_len, htable=1024, kind="", magic=True, out=None):
    """One ez_compress_batch call -> (route, CompressedBatch), the kernel choice `kind` forced."""
    import torch

    import eazy_amd as ez

    ez.select_compress_kernel(kind)
    try:
        cb = ez.compress_batch(dev.data, dev.off, MiB, htable, max_len=max_len, append_magic=magic, out=out)
        torch.cuda.synchronize()
        return ez.compress_route_last(), cb
    finally:
        ez.select_compress_kernel("")


def slot_bytes(cb):
    st, sz, so = cb.status.cpu().numpy(), cb.sizes.cpu().numpy(), cb.slot_off.cpu().numpy()
    return st, sz, so, cb.slots.cpu().numpy()


def assert_exact(cb, want, what, only=None):
    st, sz, so, slots = slot_bytes(cb)
    for s in range(len(want)) if only is None else only:
        assert st[s] == 0, f"{what}: stream {s} status {st[s]}"
        got = slots[so[s] : so[s] + sz[s]].tobytes()
        assert got == want[s], f"{what}: stream {s} ({sz[s]} bytes, the oracle {len(want[s])}) differs from the oracle"


def assert_guards(cb, what):
    slots = cb.slots.cpu().numpy()
    so = cb.slot_off.cpu().numpy()
    assert so[0] == GUARD and len(slots) == so[-1] + GUARD
    assert (slots[:GUARD] == FILL).all(), f"{what}: bytes before the first slot written"
    assert (slots[so[-1] :] == FILL).all(), f"{what}: bytes after the last slot written"


# ------------------------------------------------------------------ C1: a hint larger than the batch

# (max_len, forced kind, htable, append_magic) -> route, block 1 MiB, 40 streams of <= 4096 bytes.
# Read from ez_k1_lean.hip launch_lean (8-lane groups: max_len > 4096; the 40-byte
# judgement: max_len <= 16384), split_table / split_table_words
# (u16 table: max_len <= kMaxT16 = 65536; u32 table: <= kMaxT32 = 2^19 and 2 max_len <= block),
# launch_compress_split (single Writes on the u32 table: launch_long), chunk_applies (K1c:
# count <= 1024, max_len >= 2 C = 65536, not with 'l' forced); ez_compress_spec.hip spec_applies
# (K1x: max_len >= 64 KiB where K1s does not apply); ez_compress.hip launch_general (kPLdsMax =
# 16384: stream staged in LDS; above: the LDS window; 0: the multi-Write / 64-bit variant on the
# global view; kHtLdsMax = 4096: larger tables in global scratch) and compress_variant.
EXACT = 4096
C1_ROUTES = [
    ((EXACT, "", 1024, True), "s:lean g16 fw40"),
    ((4097, "", 1024, True), "s:lean g8 fw40"),
    ((16384, "", 1024, True), "s:lean g8 fw40"),
    ((16385, "", 1024, True), "s:lean g8 fw24"),
    ((65536, "", 1024, True), "s:lean g8 fw24"),
    ((65537, "", 1024, True), "l:k1c"),
    ((65537, "l", 1024, True), "l"),
    ((1 << 19, "", 1024, True), "l:k1c"),
    ((1 << 19, "l", 1024, True), "l"),
    (((1 << 19) + 1, "", 1024, True), "x"),
    ((1 << 20, "", 1024, True), "x"),
    ((0, "", 1024, True), "w:view"),
    ((0, "", 8192, True), "w:view+gtab"),
    ((EXACT, "", 8192, True), "w:pl+gtab"),
    ((16384, "", 8192, True), "w:pl+gtab"),
    ((16385, "", 8192, True), "w:win+gtab"),
    ((EXACT, "", 1024, False), "s:lean g16 fw40"),
    ((65536, "", 1024, False), "s:lean g8 fw24"),
]


@pytest.mark.gpu
def test_hint_larger_than_the_batch(cuda):
    """One ragged batch of small streams under every hint a caller with a fixed max_len could
    pass: each call takes the route the table names, every status is 0 and every slot holds the
    oracle's bytes -- 8-lane groups and the 24-byte judgement on tiny streams, K1L / K1c / K1x on
    streams that fit one chunk, edge slots sized for streams far longer than the ones in them,
    and max_len = 0."""
    bufs = hint_streams()
    dev = DevBatch(cuda, bufs)
    got_routes = []
    for (max_len, kind, htable, magic), route in C1_ROUTES:
        what = f"max_len {max_len} kind {kind!r} htable {htable} magic {magic}"
        got, cb = run_k1(dev, max_len, htable, kind, magic)
        got_routes.append((max_len, kind, htable, magic, got))
        print(f"C1 route: {what} -> {got}")
        assert got == route, f"{what}: route {got!r}, the table says {route!r}"
        assert_exact(cb, oracle_of(bufs, htable, magic), what)


# ------------------------------------------------------------------ C2: n == max_len


@pytest.mark.gpu
@pytest.mark.parametrize(
    "h,htable",
    [(4096, 1024), (4097, 1024), (16384, 1024), (16385, 1024), (65536, 1024), (65537, 1024), (1 << 19, 1024),
     (4096, 8192), (16384, 8192)],
)
def test_stream_exactly_the_hint(cuda, h, htable):
    """A stream of exactly max_len bytes (logs with planted matches) among five short ones is
    accepted: every status 0, every stream the oracle's."""
    from eazy_amd import synth

    d = synth.logs(113, 9000).tobytes()
    bufs = (d[:11], d[11:2011], _log_planted(h, h), d[2011:2016], d[2016:5000], d[5000:5013])
    dev = DevBatch(cuda, bufs)
    route, cb = run_k1(dev, h, htable)
    print(f"C2 route: max_len {h} htable {htable} -> {route}")
    assert_exact(cb, oracle_of(bufs, htable), f"max_len {h} htable {htable} ({route})")


# ------------------------------------------------------------------ C3: n > max_len

KiB = 1 << 10
C3_CASES = [
    # id, forced kind, hint, htable, route
    ("lean-g16", "", 4096, 1024, "s:lean g16 fw40"),
    ("lean-g8", "", 8192, 1024, "s:lean g8 fw40"),
    ("parse-t32", "S", 4096, 1024, "s:parse t32"),
    ("k1l", "l", 100 * KiB, 1024, "l"),
    ("k1c", "", 128 * KiB, 1024, "l:k1c"),
    ("k1x", "x", 128 * KiB, 1024, "x"),
    ("general-pl-4096", "w", 4096, 1024, "w:pl"),
    ("general-pl-16384", "w", 16384, 1024, "w:pl"),
    ("general-win", "w", 20000, 1024, "w:win"),
    ("auto-htable-8192", "", 4096, 8192, "w:pl+gtab"),
]


@functools.lru_cache(maxsize=None)
def refusal_streams(hint):
    """9 streams: 0, 4 and 8 are longer than the hint (hint + 1, 3 hint + 5, hint + 1 bytes), the
    other six log slices of at most hint bytes, one of exactly hint bytes."""
    from eazy_amd import synth

    d = synth.logs(127 + hint, 5 * hint + 4096).tobytes()
    lens = {0: hint + 1, 4: 3 * hint + 5, 8: hint + 1, 1: hint // 2 + 3, 2: hint, 3: 19, 5: hint - 1, 6: hint // 3, 7: 5}
    bufs, at = [], 0
    for s in range(9):
        n = lens[s]
        if s == 2:
            bufs.append(_log_planted(131 + hint, n))
            continue
        bufs.append((d + d)[at : at + n])
        at = (at + n) % len(d)
    return tuple(bufs)


REFUSED = (0, 4, 8)
GOOD = (1, 2, 3, 5, 6, 7)


def check_refusals(cb, want, what, refused, status):
    """The refused streams: `status`, size 0, their slots untouched; the others the oracle's;
    nothing outside the slots; the packing holds exactly the good streams."""
    import torch

    import eazy_amd as ez

    st, sz, so, slots = slot_bytes(cb)
    good = [s for s in range(len(want)) if s not in refused]
    for s in refused:
        assert st[s] == status, f"{what}: stream {s} status {st[s]}, expected {status}"
        assert sz[s] == 0, f"{what}: refused stream {s} has size {sz[s]}"
        assert (slots[so[s] : so[s + 1]] == FILL).all(), f"{what}: refused stream {s}'s slot was written"
    assert_exact(cb, want, what, only=good)
    assert_guards(cb, what)
    packed, poff = ez.pack(cb)
    torch.cuda.synchronize()
    po = poff.cpu().numpy()
    assert packed[: po[-1]].cpu().numpy().tobytes() == b"".join(want[s] for s in good), f"{what}: packing"
    for s in refused:
        assert po[s + 1] == po[s], f"{what}: packed entry of refused stream {s} is not empty"


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,hint,htable,route", C3_CASES, ids=[c[0] for c in C3_CASES])
def test_stream_longer_than_the_hint(cuda, name, kind, hint, htable, route):
    """Streams longer than max_len at the batch's first, middle and last position, on every
    route: EZ_EINVAL, size 0 and an untouched slot for them, the oracle's bytes for the six
    others (one of exactly max_len bytes), no byte outside the slots, and a packing of exactly
    the six."""
    import eazy_amd as ez

    bufs = refusal_streams(hint)
    dev = DevBatch(cuda, bufs)
    got, cb = run_k1(dev, hint, htable, kind, out=dev.guarded())
    print(f"C3 route: {name} max_len {hint} -> {got}")
    assert got == route, f"{name}: route {got!r}, expected {route!r}"
    want = [None] * 9
    for s, w in zip(GOOD, oracle_of(tuple(bufs[s] for s in GOOD), htable)):
        want[s] = w
    check_refusals(cb, want, f"{name} ({got})", REFUSED, ez.EINVAL)


# ------------------------------------------------------------------ C4: multi-Write hints


@functools.lru_cache(maxsize=None)
def multi_write_streams():
    """12 streams of 1 - 8 Writes (empty ones, ones shorter than a hash among them), each
    stream at most 3000 bytes; stream 7 is exactly 3000 bytes, stream 4 has 8 Writes."""
    from eazy_amd import synth

    rng = np.random.default_rng(137)
    d = synth.logs(139, 1 << 16).tobytes()
    nws = [1, 3, 2, 5, 8, 1, 4, 2, 7, 6, 2, 3]
    streams, at = [], 0
    for s, k in enumerate(nws):
        budget = 3000
        ws = []
        for j in range(k):
            n = int(rng.choice([0, 1, 3, 5, 17, int(rng.integers(0, 900))]))
            n = min(n, budget)
            if s == 7 and j == k - 1:
                n = budget
            ws.append(d[at : at + n])
            at += n
            budget -= n
        streams.append(tuple(ws))
    assert max(sum(len(w) for w in ws) for ws in streams) == 3000 and len(streams[4]) == 8
    return tuple(streams)


def run_writes(cuda, streams, kind, max_len, max_writes):
    """ez_compress_batch_writes into guarded slots -> (route, CompressedBatch)."""
    import torch

    import eazy_amd as ez

    data = b"".join(b"".join(ws) for ws in streams)
    in_off, w_idx, w_end = [0], [0], []
    pos = 0
    for ws in streams:
        for w in ws:
            pos += len(w)
            w_end.append(pos)
        in_off.append(pos)
        w_idx.append(len(w_end))
    t = lambda a: torch.tensor(a, dtype=torch.int64, device=cuda)
    dd = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)
    io, wi = t(in_off), t(w_idx)
    n, nw = io[1:] - io[:-1], wi[1:] - wi[:-1]
    cap = (n + (n >> 2) + 32 + 5 * nw + 15) & ~15  # ez_compress_bound + 5 bytes per Write (include/eazy.h)
    so = torch.cat([torch.zeros(1, dtype=torch.int64, device=cuda), torch.cumsum(cap, 0)]) + GUARD
    out = ez.CompressedBatch(
        torch.full((int(so[-1].item()) + GUARD,), FILL, dtype=torch.uint8, device=cuda),
        so,
        torch.full((len(streams),), -1, dtype=torch.int64, device=cuda),
        torch.full((len(streams),), -1, dtype=torch.int32, device=cuda),
    )
    ez.select_compress_kernel(kind)
    try:
        cb = ez.compress_batch_writes(dd, io, wi, t(w_end), MiB, 1024, max_len=max_len, max_writes=max_writes, out=out)
        torch.cuda.synchronize()
        return ez.compress_route_last(), cb
    finally:
        ez.select_compress_kernel("")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("", "s:parse t16 mw"), ("w", "w:view")], ids=["auto", "general"])
def test_multi_write_hints(cuda, kind, route):
    """Multi-Write batches under stated hints, on K1s (k1_parse) and on the general kernel:
    (a) overstated max_len and max_writes change nothing; (b) a stream whose Writes total
    max_len + 1 bytes is refused (EZ_EINVAL, size 0), one of exactly max_len accepted; (c) a
    stream with more Writes than max_writes is refused with EZ_ESTUCK (the status of k1_parse's
    record-capacity guard: its Writes' end markers have no record reserved), nothing written
    outside its slot, the others exact."""
    import eazy_amd as ez

    streams = multi_write_streams()
    want = [orc.compress(MiB, 1024, list(ws)) for ws in streams]
    # (a)
    got, cb = run_writes(cuda, streams, kind, 65536, 64)
    print(f"C4 route: kind {kind!r} -> {got}")
    assert got == route
    assert_exact(cb, want, f"overstated hints ({got})")
    assert_guards(cb, "overstated hints")
    # (b) stream 9 grows to max_len + 1 bytes; stream 7 is exactly max_len
    long9 = streams[9][:-1] + (streams[9][-1] + bytes(3001 - sum(len(w) for w in streams[9])),)
    sb = streams[:9] + (long9,) + streams[10:]
    got, cb = run_writes(cuda, sb, kind, 3000, 8)
    assert got == route
    check_refusals(cb, [None if s == 9 else want[s] for s in range(12)], f"total max_len + 1 ({got})", (9,), ez.EINVAL)
    # (c) max_writes states 2: every stream but 4 (8 Writes) keeps its first two Writes
    sc = tuple(ws if s == 4 else ws[:2] for s, ws in enumerate(streams))
    wc = [None if s == 4 else orc.compress(MiB, 1024, list(ws)) for s, ws in enumerate(sc)]
    got, cb = run_writes(cuda, sc, kind, 3000, 2)
    assert got == route
    check_refusals(cb, wc, f"8 Writes under max_writes 2 ({got})", (4,), ez.ESTUCK)


# ------------------------------------------------------------------ C5: the decode hint


@pytest.mark.gpu
def test_decode_hint_any_value(cuda):
    """K2 on the automatic route under max_len 1, 4096, the exact largest slot and 2^30: the
    hint picks the decoder only -- sizes, statuses and bytes are the same for every value and the
    bytes are the input (the small ragged batch, and 4 x 256 KiB of logs)."""
    import torch

    import eazy_amd as ez

    for bufs in (hint_streams(), big_streams()):
        dev = DevBatch(cuda, bufs)
        exact = int(dev.lens.max())
        _, cb = run_k1(dev, exact)
        assert int(cb.status.abs().sum()) == 0
        packed, poff = ez.pack(cb)
        first = None
        for hint in (exact, 1, 4096, 1 << 30):
            out, sizes, status = ez.decompress_batch(packed, poff, dev.off, max_len=hint)
            torch.cuda.synchronize()
            res = (out[: len(dev.host)].cpu().numpy().tobytes(), sizes.cpu().tolist(), status.cpu().tolist())
            what = f"{len(bufs)} streams, max_len {hint} ({ez.decompress_kernel_last()})"
            if first is None:
                first = res
                assert res[2] == [0] * len(bufs), what
                assert res[1] == dev.lens.tolist(), what
                assert res[0] == dev.host.tobytes(), what
            else:
                assert res[2] == first[2] and res[1] == first[1], what
                assert res[0] == first[0], what
