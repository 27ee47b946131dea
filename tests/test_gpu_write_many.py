"""ez_writer_write_many: one Write on each of many Writer handles in one device call.

The Writes K1L takes on its LDS path share one launch, a block of threads per handle, each block
reading its own handle's ring, table and sizes from a descriptor; every other Write runs on its
handle's own path inside the same call.  A block that read another handle's descriptor, ring or
meta words would still write a stream that decodes; only its bytes differ from Go's.  So every
Write's bytes are held to the oracle's (oracle/eazy_oracle.c, Write by Write), on the hand-built
sequences of tests/k1w_inputs.py run in lockstep, one handle per sequence."""

import ctypes as C

import numpy as np
import pytest

import k1w_inputs as kw
import oracle as orc
from test_gpu_k1_handle import first_difference, sequence
from test_gpu_k1_hints import FILL, GUARD

P32 = 1 << 32
VP = C.c_void_p


class Lib:
    def __init__(self):
        import eazy_amd as ez

        self.ez, self.L = ez, ez._lib()
        self.L.ez_writer_write_many.argtypes = [VP, C.c_size_t, VP, VP, VP, C.c_size_t, VP, VP]
        self.L.ez_writer_write_many_last.argtypes = [VP]
        self.L.ez_writer_set_position.argtypes = [VP, C.c_int64]
        self.made = []

    def new(self, block, htable, magic=True):
        h = VP()
        assert self.L.ez_writer_new(block, htable, 0, C.byref(h)) == 0
        if not magic:
            self.L.ez_writer_set_append_magic(h, 0)
        self.made.append(h)
        return h

    def free(self):
        for h in self.made:
            self.L.ez_writer_free(h)
        self.made = []

    def counts(self):
        c = (C.c_uint64 * 2)()
        assert self.L.ez_writer_write_many_last(c) == 0
        return int(c[0]), int(c[1])

    def write(self, h, p):
        """ez_writer_write -> (status, bytes)."""
        cap = self.ez.compress_bound(len(p))
        out = np.full(cap + GUARD, FILL, np.uint8)
        n = C.c_size_t()
        st = self.L.ez_writer_write(h, bytes(p), len(p), VP(out.ctypes.data), cap, C.byref(n))
        return st, out[: n.value].tobytes()

    def many(self, hs, ps, short=0, ends=None):
        """One ez_writer_write_many call: the output buffer is the sum of the bounds long (cap
        `short` bytes less) with a guard after it.  -> (return code, every handle's bytes, its
        status, the whole buffer); the guard and the input are unchanged."""
        k = len(ps)
        need = sum(self.ez.compress_bound(len(p)) for p in ps)
        src = np.frombuffer(b"".join(ps) + b"\x00", np.uint8).copy()
        keep = src.copy()
        out = np.full(need + GUARD, FILL, np.uint8)
        e = np.cumsum([len(p) for p in ps] + [0]).astype(np.uint64)[:k] if ends is None else np.array(ends, np.uint64)
        e = np.concatenate([e, np.zeros(1, np.uint64)])  # (never empty: a pointer to pass)
        oe = np.zeros(k + 1, np.uint64)
        st = np.full(k + 1, -7, np.int32)
        arr = (VP * max(k, 1))(*[h if h is None else h.value for h in hs])
        rc = self.L.ez_writer_write_many(arr, k, VP(src.ctypes.data), VP(e.ctypes.data), VP(out.ctypes.data), need - short,
                                         VP(oe.ctypes.data), VP(st.ctypes.data))
        assert (out[need:] == FILL).all(), "the guard after the output was written"
        assert np.array_equal(src, keep), "the input was written"
        bounds = [0] + [int(v) for v in oe[:k]]
        return rc, [out[a:b].tobytes() for a, b in zip(bounds, bounds[1:])], [int(v) for v in st[:k]], out


@pytest.fixture()
def lib(cuda):
    lb = Lib()
    yield lb
    lb.ez.select_compress_kernel("")
    lb.free()


def shares(block, htable, start, n, forced=False):
    """The issue's rule for a Write that shares the launch."""
    return not forced and 16 <= n <= kw.LDS_WRITE and htable <= 4096 and block <= (1 << 26) and start + n <= P32


def lines(seed, count, lo=40, hi=200):
    """count seeded log lines of lo .. hi bytes: words of a small vocabulary and numbers."""
    rng = np.random.default_rng(seed)
    words = [b"GET", b"POST", b"/api/v1/items", b"/index.html", b"status=200", b"status=404", b"user=", b"latency_ms=", b"conn", b"tenant-", b"INFO", b"WARN", b"retry", b"ok"]
    out = []
    for _ in range(count):
        n = int(rng.integers(lo, hi + 1))
        b = b"2026-01-01T00:00:%02d " % int(rng.integers(0, 60))
        while len(b) < n:
            b += words[int(rng.integers(0, len(words)))] + b"%d " % int(rng.integers(0, 100000))
        out.append(b[:n])
    return out


# ------------------------------------------------------------------ 1: lockstep over the hand-built edges


@pytest.mark.gpu
@pytest.mark.parametrize("g", ["R1", "R2", "R3", "R4", "R6"])
def test_many_lockstep(lib, g):
    """Every sequence of the group on a handle of its own (its block and table size); step t is one
    call with the t-th Write of every sequence that still has one.  Every Write's bytes are the
    oracle's, and every Write of 16 .. 49,152 bytes shared the launch: ring wraps, candidates on both
    sides of the Write's start, the staged extent's ends, Writes of 49,151 .. 49,153 bytes and the
    table carried from launch to launch, in one grid of blocks with differing block and table sizes."""
    cases = kw.group(g)
    seqs = [sequence(c, 0, c.htable) for c in cases]
    hs = [lib.new(c.block, c.htable) for c in cases]
    starts = [c.starts() for c in cases]
    in_launch = 0
    for t in range(max(len(ws) for ws, _ in seqs)):
        live = [i for i, (ws, _) in enumerate(seqs) if t < len(ws)]
        for i in live:
            if t in cases[i].pos:
                assert lib.L.ez_writer_set_position(hs[i], cases[i].pos[t]) == 0
        ps = [seqs[i][0][t] for i in live]
        rc, got, st, _ = lib.many([hs[i] for i in live], ps)
        route = lib.ez.compress_route_last()
        assert rc == 0 and st == [0] * len(live), f"{g} step {t}: code {rc}, statuses {sorted(set(st))} on {route!r}"
        for i, b in zip(live, got):
            c, want = cases[i], seqs[i][1][t]
            assert b == want, (
                f"{c.name} (block {c.block}, htable {c.htable}): Write {t} ({len(seqs[i][0][t])} bytes at position {starts[i][t]}) "
                f"as handle {live.index(i)} of {len(live)} on {route!r}: {len(b)} bytes, the oracle {len(want)}; {first_difference(b, want)}"
            )
        exp = sum(shares(cases[i].block, cases[i].htable, starts[i][t], len(seqs[i][0][t])) for i in live)
        assert lib.counts() == (exp, len(live) - exp), f"{g} step {t}"
        assert route == ("hm:lds" if exp == len(live) else ("hm:lds+own" if exp else "hm:own"))
        in_launch += exp
    assert in_launch >= len(cases)


# ------------------------------------------------------------------ 2: the routes of one call


def _mix(lib):
    """[(handle, Write, the oracle's bytes, shares the launch)]: Writes of 0 .. 49,153 bytes, a table of
    8,192 entries, and R5's Write across 2^32 on a handle moved there."""
    rows = []
    body = b"".join(lines(5, 600))
    assert len(body) >= 49153
    for n in (0, 15, 16, 100, 49152, 49153):
        p = body[:n]
        rows.append((lib.new(65536, 1024), p, kw.oracle_writes(65536, 1024, [p])[0], 16 <= n <= kw.LDS_WRITE))
    p = body[100:200]
    rows.append((lib.new(65536, 8192), p, kw.oracle_writes(65536, 8192, [p])[0], False))
    c = [c for c in kw.group("R5") if c.name == "R5-ends-at-2^32+1"][0]
    h = lib.new(c.block, c.htable)
    assert lib.L.ez_writer_set_position(h, c.pos[0]) == 0
    st, b = lib.write(h, c.writes[0])
    assert st == 0 and b == c.comps[0]
    assert c.starts()[1] < P32 < c.starts()[1] + len(c.writes[1])
    rows.append((h, c.writes[1], c.comps[1], False))
    return rows


@pytest.mark.gpu
def test_many_route_mix(lib):
    """Writes of 0, 15, 16, 100, 49,152 and 49,153 bytes, a table of 8,192 entries and a Write across
    2^32 in one call: the oracle's bytes, 3 Writes in the launch and 5 on their own path,
    "hm:lds+own"; the qualifying Writes alone "hm:lds"; everything "hm:own" with the general kernel
    forced."""
    rows = _mix(lib)
    rc, got, st, _ = lib.many([r[0] for r in rows], [r[1] for r in rows])
    assert rc == 0 and st == [0] * len(rows)
    for j, (r, b) in enumerate(zip(rows, got)):
        assert b == r[2], f"handle {j} ({len(r[1])} bytes): {first_difference(b, r[2])}"
    assert lib.counts() == (3, 5) and [r[3] for r in rows].count(True) == 3
    assert lib.ez.compress_route_last() == "hm:lds+own"

    rows = [r for r in _mix(lib) if r[3]]
    rc, got, st, _ = lib.many([r[0] for r in rows], [r[1] for r in rows])
    assert rc == 0 and got == [r[2] for r in rows]
    assert lib.counts() == (3, 0) and lib.ez.compress_route_last() == "hm:lds"

    rows = _mix(lib)
    lib.ez.select_compress_kernel("w")
    try:
        rc, got, st, _ = lib.many([r[0] for r in rows], [r[1] for r in rows])
    finally:
        lib.ez.select_compress_kernel("")
    assert rc == 0 and got == [r[2] for r in rows]
    assert lib.counts() == (0, 8) and lib.ez.compress_route_last() == "hm:own"


# ------------------------------------------------------------------ 3, 4: counts, and the single path

BLOCK, HTABLE, ROUNDS = 1024, 256, 3


def _rounds(count):
    """Handle j's line of each round."""
    ls = lines(1000 + count, count * ROUNDS)
    return [[ls[r * count + j] for r in range(ROUNDS)] for j in range(count)]


def _segments(count, j, ws):
    """Handle j's Writes by stream: every third handle is reset before round 2."""
    return [ws[:1], ws[1:]] if j % 3 == 0 else [ws]


def _run_rounds(lib, count, single):
    """Three rounds of one line per handle -> (each handle's bytes per round, its is_reset state after
    each round); single: through ez_writer_write handle by handle, else ez_writer_write_many."""
    ws = _rounds(count)
    hs = [lib.new(BLOCK, HTABLE, magic=j % 5 != 0) for j in range(count)]
    outs, states = [[] for _ in hs], []
    for r in range(ROUNDS):
        if r == 1:
            for j in range(0, count, 3):
                assert lib.L.ez_writer_reset(hs[j]) == 0
        ps = [ws[j][r] for j in range(count)]
        if single:
            got = []
            for h, p in zip(hs, ps):
                st, b = lib.write(h, p)
                assert st == 0
                got.append(b)
        else:
            rc, got, st, _ = lib.many(hs, ps)
            assert rc == 0 and st == [0] * count
            assert lib.counts() == (count, 0)
        for j, b in enumerate(got):
            outs[j].append(b)
        states.append([lib.L.ez_writer_is_reset(h) for h in hs])
    return ws, outs, states


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 2, 5, 300])
def test_many_counts(lib, count):
    """0, 1, 2, 5 and 300 handles (more blocks than the chip has CUs) at block 1,024 and table 256,
    a different 40 .. 200-byte line each for three rounds, every third handle reset before round 2
    (pristine and written handles in one launch), AppendMagic off on every fifth: each handle's bytes
    are the oracle's for its streams, and each stream decodes to its lines."""
    if count == 0:
        rc, got, st, out = lib.many([], [])
        assert rc == 0 and got == [] and (out == FILL).all() and lib.counts() == (0, 0)
        assert lib.L.ez_writer_write_many(None, 0, None, None, None, 0, None, None) == 0
        return
    ws, outs, _ = _run_rounds(lib, count, single=False)
    for j in range(count):
        segs = _segments(count, j, ws[j])
        want = b"".join(orc.compress(BLOCK, HTABLE, s, append_magic=j % 5 != 0) for s in segs)
        got = b"".join(outs[j])
        assert got == want, f"handle {j} of {count}: {first_difference(got, want)}"
        at = 0
        for s in segs:
            n = len(orc.compress(BLOCK, HTABLE, s, append_magic=j % 5 != 0))
            assert orc.decompress(got[at : at + n])[0] == b"".join(s), f"handle {j} of {count}"
            at += n


@pytest.mark.gpu
def test_many_equals_single_writes(lib):
    """The same rounds through ez_writer_write on fresh handles: identical bytes Write by Write and
    identical ez_writer_is_reset states."""
    _, many, sm = _run_rounds(lib, 5, single=False)
    _, one, s1 = _run_rounds(lib, 5, single=True)
    assert many == one and sm == s1


# ------------------------------------------------------------------ 5: refusals


@pytest.mark.gpu
def test_many_refusals_leave_no_trace(lib):
    """A handle named twice, a NULL handle, decreasing ends and a cap one byte short: each returns
    its code with nothing written to out, and the next valid call gives the bytes of a history without
    the refused call."""
    ls = lines(77, 8)
    hs = [lib.new(BLOCK, HTABLE) for _ in range(3)]
    rc, got, st, _ = lib.many(hs, ls[:3])
    assert rc == 0
    hist = [[ls[j]] for j in range(3)]
    ez = lib.ez
    refused = [
        ("twice", [hs[0], hs[1], hs[0]], ls[3:6], 0, None, ez.EINVAL),
        ("null", [hs[0], None, hs[2]], ls[3:6], 0, None, ez.EINVAL),
        ("ends", hs, ls[3:6], 0, [len(ls[3]), len(ls[3]) - 1, len(ls[3]) + 50], ez.EINVAL),
        ("cap", hs, ls[3:6], 1, None, ez.ENOSPC),
    ]
    for name, hh, ps, short, ends, code in refused:
        rc, _, st, out = lib.many(hh, ps, short=short, ends=ends)
        assert rc == code, name
        assert (out == FILL).all(), f"{name}: out was written"
        assert st == [-7] * 3, f"{name}: status was written"
    assert lib.L.ez_writer_write_many(None, 3, None, None, None, 0, None, None) == ez.EINVAL
    rc, got, st, _ = lib.many(hs, ls[5:8])
    assert rc == 0
    for j in range(3):
        want = kw.oracle_writes(BLOCK, HTABLE, hist[j] + [ls[5 + j]])[1]
        assert got[j] == want, f"handle {j} after the refused calls: {first_difference(got[j], want)}"


@pytest.mark.gpu
def test_many_staging_is_released_and_taken_again(lib):
    """ez_release_cached frees the call's leased staging, device buffer and records; the next call
    takes new ones and goes on with every handle's stream."""
    ls = lines(78, 8)
    hs = [lib.new(BLOCK, HTABLE) for _ in range(4)]
    rc, first, _, _ = lib.many(hs, ls[:4])
    assert rc == 0
    lib.ez.release_cached(0)
    rc, got, _, _ = lib.many(hs, ls[4:])
    assert rc == 0 and lib.counts() == (4, 0)
    for j in range(4):
        want = kw.oracle_writes(BLOCK, HTABLE, [ls[j], ls[4 + j]])
        assert [first[j], got[j]] == want, f"handle {j}"


# ------------------------------------------------------------------ 6: the Python mirror


class Sink:
    def __init__(self, take=None):
        self.calls, self.take = [], take

    def write(self, b):
        self.calls.append(bytes(b))
        if self.take is not None and len(self.calls) == 2:
            return min(self.take, len(b))  # a short write: the stream restarts
        return len(b)


def _mirror(ez, many):
    sinks = [Sink(take=3 if j == 5 else None) for j in range(8)]
    ws = [ez.Writer(s, BLOCK, HTABLE) for s in sinks]
    ws[2].FlushThreshold = 64
    ws[6].AppendMagic = False
    ls = lines(31, 8 * 4, lo=20, hi=90)
    took = []
    for r in range(4):
        ps = [ls[r * 8 + j] for j in range(8)]
        took.append(ez.write_many(ws, ps) if many else [w.Write(p) for w, p in zip(ws, ps)])
    for w in ws:
        w.Flush()
    return [s.calls for s in sinks], took


@pytest.mark.gpu
def test_many_python_mirror(lib):
    """write_many over 8 Writers with recording sinks, one with FlushThreshold 64 and one whose sink
    takes a short write: every sink's call list is that of the same Writes through Write."""
    calls_many, took_many = _mirror(lib.ez, True)
    calls_one, took_one = _mirror(lib.ez, False)
    assert took_many == took_one
    assert calls_many == calls_one
    assert all(len(c) >= 2 for c in calls_many)
