"""k1_lean's two window loops (ez_k1_lean.hip, lean_run): the interior loop, which a wave runs
while every one of its groups is live, has room for a record and i + kIn <= n, and the general
loop it hands over to.  kIn = G + CAP - 1, G the lanes per stream and CAP the judgement's
forward cap: 55 on "s:lean g16 fw40", 47 on "s:lean g8 fw40", 31 on "s:lean g8 fw24".

A window that runs in the wrong loop, or a count whose limit the wrong loop dropped, still
writes a stream that decodes back; only its bytes differ from Go's.  So every batch here is
compared byte for byte (sizes, statuses, slot bytes) with the C oracle, on inputs built by hand
at the smallest shapes at which the hand-over can go wrong.  A wave stays in the interior loop
only while all of its 64 / G streams are interior, and does not return to it: the batches that
aim at the hand-over hold each stream eight times in a row, so the 4 or 8 groups of a wave take
the same windows and leave the interior in the same one; the mixed batches hold streams of very
different lengths side by side, so a wave leaves the interior early or never enters it.

The record area cannot be filled by a hand-built input: a stream longer than max_len is refused
when it is opened, every record moves `done` on by at least 6 bytes, and the area holds
max_len / 6 + 1 records, so nrec < rcap holds at every window of an accepted stream (the test
of it stays in the loops as the guard it was).

The GPU tests are marked one by one: the first two tests run on the CPU."""

import functools

import numpy as np
import pytest

import k1_inputs as ki
import oracle as orc
from test_gpu_k1_edges import run_route
from test_gpu_k1_hints import DevBatch, _log_planted, check_refusals, oracle_of, run_k1

MiB = 1 << 20
HTABLE = 1024

# (route, max_len, G, CAP): launch_lean's choices (8-lane groups above 4,096 bytes, the 40-byte
# judgement up to 16,384); lean_run's kIn = G + CAP - 1
LEAN = [("s:lean g16 fw40", 4096, 16, 40), ("s:lean g8 fw40", 8192, 8, 40), ("s:lean g8 fw24", 32768, 8, 24)]
LEAN_IDS = [r[0].replace(" ", "-") for r in LEAN]
every_lean_route = pytest.mark.parametrize("lean", LEAN, ids=LEAN_IDS)
REPEAT = 8  # a stream this often in a row fills whole waves on every route (4 or 8 streams per wave)


def k_in(G, CAP):
    return G + CAP - 1


# ------------------------------------------------------------------ stream lengths


def lengths_of(max_len, G, CAP):
    """The issue's lengths for the 16-lane route (4, 5, 19, 20, 55, 56, 57, 71, 72, 73, 96, 128,
    4095, 4096), at the same offsets around every route's own bound: the bound itself (the first
    window is the last interior one), one window of G further on, and one less and one more."""
    b = k_in(G, CAP)
    return sorted({4, 5, 19, 20, b - 1, b, b + 1, b + 2, b + G - 1, b + G, b + G + 1, b + G + 2, 96, 128, 4095, 4096, max_len - 1, max_len})


@functools.lru_cache(maxsize=None)
def length_streams(max_len, G, CAP):
    """[(name, bytes)]: per length four streams of incompressible bytes (no accept: i advances by
    G to the bound) and four of logs with planted copies, runs and zero runs."""
    rng = np.random.default_rng(1000 + G + CAP)
    out = []
    for n in lengths_of(max_len, G, CAP):
        for k in range(4):
            out.append((f"{n} random bytes #{k}", rng.integers(1, 256, n, dtype=np.uint8).tobytes()))
        for k in range(4):
            out.append((f"{n} bytes of logs #{k}", _log_planted(17 * n + k, max(n, 200))[:n]))
    return out


# ------------------------------------------------------------------ content at the hand-over


def switch_fwd(b, L, lane, d, kin):
    """An anchor copy ends at A, the next window's i; `lane` filler bytes; a window match of L
    bytes, accepted in that window by lane `lane`; the stream ends at A + kin + d: the window is
    the last interior one for d = 0, the first general one for d = -1.  With lane = G - 1 and
    L = CAP + d the match is at its cap and ends with the stream.  The source is followed by the
    stream's first 3 bytes, which in a row of equal streams also follow the stream's end: a count
    that is not held to n there finds 3 bytes more than Go."""
    b.fill(2)
    src = b.fill(L)
    b.raw(bytes(b.d[0:3]))
    asrc = b.fill(14) + 3
    b.anchor(asrc, pend=5)
    A = b.pos()
    b.fill(lane)
    x = b.copy(src, L)
    b.accept("window", x, src, x, x + L)
    tail = A + kin + d - b.pos()
    assert tail >= 0, (L, lane, d, kin)
    b.fill(tail)


def jump(b, L, lane, t):
    """The same match deep in the interior (L >= 60), ending t bytes before the stream's end
    (t = 0: the exact extension's limit is the stream's end, with the same lure behind it)."""
    b.fill(2)
    src = b.fill(L)
    b.raw(bytes(b.d[0:3]))
    asrc = b.fill(14) + 3
    b.anchor(asrc, pend=5)
    A = b.pos()
    b.fill(lane)
    x = b.copy(src, L)
    b.accept("window", x, src, x, x + L)
    b.fill(t)


def zeros_to_end(b, Z):
    """21 filler bytes and Z zero bytes up to the stream's end: the zero token, found at 22."""
    b.fill(21)
    z = b.raw(bytes(Z))
    b.accept("zeros", z + 1, z, z, z + Z)


def fwd_no_room(b, CAP, lane, tail):
    """A window match of CAP + 1 bytes at `at` (Go inserts at + 1), `lane` filler bytes, and the
    copy's bytes 1 .. CAP again: the candidate at + 1 is CAP bytes below done, so the forward
    count is at its cap with no room left (done - cand = CAP)."""
    b.fill(2)
    u = b.fill(CAP + 1)
    asrc = b.fill(14) + 3
    b.anchor(asrc, pend=5)
    b.fill(3)
    at = b.copy(u, CAP + 1)
    b.accept("window", at, u, at, at + CAP + 1)
    b.fill(lane)
    if b.d[-1] == b.d[at]:
        raise ki.Retry
    x = b.raw(bytes(b.d[at + 1 : at + 1 + CAP]))
    b.accept("window", x, at + 1, x, x + CAP)
    b.fill(tail)


def period_from_0(b, per, R, tail):
    """`per` fresh bytes and R more of that period: a run accepted in the first window with
    candidate 0 (the empty table entry's twin)."""
    b.fill(per)
    x = b.copy(0, R)
    b.accept("runlen", x, 0, x, x + R)
    b.fill(tail)


def then_fill(fn, tail):
    def f(b):
        fn(b)
        b.fill(tail)

    return f


@functools.lru_cache(maxsize=None)
def content_cases(G, CAP):
    """The cases of one route (ki.make holds each to its intended parse by both oracles)."""
    kin = k_in(G, CAP)
    seed = [7000 + 100 * G + CAP]

    def mk(name, fn):
        seed[0] += 1
        return ki.make(f"{name} (G {G}, cap {CAP})", fn, seed[0], htable=HTABLE)

    cases = []
    # a match accepted in the last interior window, the first general one and the one before; in
    # the group's last lane also a match of CAP - 4 and of CAP - 6 bytes that ends with the stream
    # (with the 3 bytes of the lure a count not held to n stays below its cap, so the exact
    # extension does not put it right)
    for lane in (0, G - 1):
        for d in (-1, 0, 1) if lane == 0 else (-6, -4, -1, 0, 1):
            for L in sorted({min(v, kin + d - lane) for v in (6, CAP - 1, CAP + 1)}):
                cases.append(mk(f"switch lane {lane} len {L} end {d:+d}", lambda b, L=L, lane=lane, d=d: switch_fwd(b, L, lane, d, kin)))
    # a match from the interior to within the bound of the end, and to the end itself
    for L in (60, 100):
        for t in (0, 3, 4, 5, kin - G, kin - 1, kin, kin + 1):
            cases.append(mk(f"jump len {L} to {t} before the end", lambda b, L=L, t=t: jump(b, L, 2, t)))
    # a zero run to the stream's end, found in a general window (short) and in an interior one
    for Z in sorted({9, CAP + 1, CAP + 2, CAP + 3, 41, 42, 43, 49, 50, 51, 100}):
        cases.append(mk(f"{Z} zeros to the end", lambda b, Z=Z: zeros_to_end(b, Z)))
    # counts at their caps: forward with room left (the match goes on or stops right there) ...
    for lane in (0, G - 1):
        for tail in (11, 90):
            for L in (CAP, CAP + 1, CAP + 30):
                cases.append(mk(f"forward {L} lane {lane} tail {tail}", lambda b, L=L, lane=lane, tail=tail: ki.fwd(b, L, lane, tail)))
            # ... and without (the candidate CAP bytes below done)
            cases.append(mk(f"forward cap, no room, lane {lane} tail {tail}", lambda b, lane=lane, tail=tail: fwd_no_room(b, CAP, lane, tail)))
    # ... backward 8 with room left (P + 8 bytes after an anchor: lane G - 1 for P = 7, lane 0 for
    # P = 8), 9, and 8 with done in the way (no room)
    for tail in (0, 80):
        for B, P, bounded in ((8, 7, False), (8, 8, False), (9, 7, False), (9, 6, False), (8, 0, True)):
            cases.append(mk(f"backward {B} after {P}{' bounded' if bounded else ''} tail {tail}", then_fill(lambda b, B=B, P=P, bounded=bounded: ki.back(b, B, P, bounded), tail)))
    # candidates at position 0 within the first window
    for per in (1, 3, 5, G - 1):
        for R in (6, 50):
            cases.append(mk(f"period {per} run {R} from 0", lambda b, per=per, R=R: period_from_0(b, per, R, 70)))
    return tuple(cases)


def _accepts(case):
    return [e for e in case.trace if e[0] not in ("far", "short")]


@pytest.mark.parametrize("lean", LEAN, ids=LEAN_IDS)
def test_interior_inputs_are_what_they_claim(lean):
    """CPU.  The oracle alone gives the intended tokens of every case (ki.make has held both
    oracles to them); the hand-over cases sit where they claim: the accepting window starts at
    the anchor's end A, the acceptor is lane x - A, and A + kIn + d is the stream's length; the
    matches at their caps have the counts and the room they claim."""
    _, max_len, G, CAP = lean
    kin = k_in(G, CAP)
    cases = content_cases(G, CAP)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        comp = orc.compress(MiB, HTABLE, [c.data])
        assert c.py_comp == comp and ki.tokens_of(comp)[0] == c.tokens, c.name
        assert orc.decompress(comp)[0] == c.data and 4 <= len(c.data) <= max_len, c.name
        ev = _accepts(c)
        if c.name.startswith("switch"):
            w = c.name.split(" (")[0].split()
            lane, L, d = int(w[2]), int(w[4]), int(w[6])
            (_, _, _, _, A), (_, x, _, ist, iend) = ev[-2], ev[-1]
            assert x - A == lane and (ist, iend) == (x, x + L) and len(c.data) == A + kin + d, c.name
        if c.name.startswith("jump"):
            assert len(c.data) - ev[-1][4] == int(c.name.split(" (")[0].split()[4]), c.name
        if "zeros to the end" in c.name:
            assert ev[-1][0] == "zeros" and ev[-1][4] == len(c.data), c.name
        if "no room" in c.name:
            (_, _, _, _, done), (_, x, cand, ist, iend) = ev[-2], ev[-1]
            assert done - cand == CAP and iend - x == CAP and ist == x, c.name
            assert c.data[cand : cand + CAP] == c.data[x : x + CAP], c.name
        if c.name.startswith("backward"):
            B = int(c.name.split()[1])
            _, x, _, ist, _ = ev[-1]
            assert x - ist == B, c.name
            if "bounded" in c.name:
                assert ist == ev[-2][4], c.name  # done stops the count: no room
        if c.name.startswith("period"):
            assert ev[0][2] == 0 and ev[0][1] < G, c.name
    # the lanes the issue names are there: the first and the last of a group accept at a cap
    for lane in (0, G - 1):
        assert any(c.name.startswith(f"switch lane {lane} len {CAP}") or c.name.startswith(f"switch lane {lane} len {CAP + 1}") for c in cases)


def test_interior_length_streams_are_what_they_claim():
    """CPU.  The random streams of the length batches parse to one literal (no accept: the
    windows advance by G), the log streams of 128 bytes and more hold copies, and every route's
    lengths straddle its bound."""
    for _, max_len, G, CAP in LEAN:
        b = k_in(G, CAP)
        assert {b - 1, b, b + 1, b + G - 1, b + G, b + G + 1} <= set(lengths_of(max_len, G, CAP))
        for name, data in length_streams(max_len, G, CAP):
            toks = ki.tokens_of(orc.compress(MiB, HTABLE, [data]))[0]
            if "random" in name and len(data) <= 4096:
                assert toks == [("l", len(data))], name
            if "logs" in name and len(data) >= 4095:
                assert sum(t[0] == "c" for t in toks) > 5, name
    assert set(lengths_of(4096, 16, 40)) >= {4, 5, 19, 20, 55, 56, 57, 71, 72, 73, 96, 128, 4095, 4096}


# ------------------------------------------------------------------ the GPU tests


@pytest.mark.gpu
@every_lean_route
def test_lean_interior_stream_lengths(cuda, lean):
    """Streams of every length around the interior bound, four of a kind side by side."""
    route, max_len, G, CAP = lean
    assert run_route(cuda, "lengths around the bound", length_streams(max_len, G, CAP), MiB, HTABLE, "", max_len, route) == route


@pytest.mark.gpu
@every_lean_route
def test_lean_interior_content_in_step(cuda, lean):
    """Every content case eight times in a row: the groups of a wave run the same windows, so the
    wave is in the interior loop up to the very window the case aims at."""
    route, max_len, G, CAP = lean
    named = [(f"{c.name} #{k}", c.data) for c in content_cases(G, CAP) for k in range(REPEAT)]
    assert run_route(cuda, "content cases in step", named, MiB, HTABLE, "", max_len, route) == route


@functools.lru_cache(maxsize=None)
def mixed_streams(max_len, G, CAP):
    """One long compressible stream beside streams of 4, 60 and 2,000 bytes (a group in its tail
    or dead while the others are interior), an empty stream and one below 4 bytes in the middle,
    then every content case once, each beside its neighbours; the count is no multiple of 8."""
    rng = np.random.default_rng(2000 + G + CAP)
    rnd = lambda n: rng.integers(1, 256, n, dtype=np.uint8).tobytes()
    out = [("logs 4096", _log_planted(301, 4096)), ("random 4", rnd(4)), ("random 60", rnd(60)), ("random 2000", rnd(2000)),
           ("logs 3000", _log_planted(302, 3000)), ("logs 300", _log_planted(303, 300)), ("empty", b""), ("random 2", rnd(2)),
           ("logs 4095", _log_planted(304, 4095)), ("logs 100", _log_planted(305, 200)[:100]), (f"random {k_in(G, CAP)}", rnd(k_in(G, CAP))),
           ("logs max_len", _log_planted(306, max_len)), ("logs 2000", _log_planted(307, 2000))]
    out += [(c.name, c.data) for c in content_cases(G, CAP)]
    while len(out) % 8 in (0, 4):
        out.append((f"random {7 + len(out)}", rnd(7 + len(out))))
    return out


@pytest.mark.gpu
@every_lean_route
def test_lean_interior_mixed_waves(cuda, lean):
    """Waves whose groups differ: streams of very different lengths side by side."""
    route, max_len, G, CAP = lean
    named = mixed_streams(max_len, G, CAP)
    assert len(named) % (64 // G) != 0
    assert run_route(cuda, "mixed waves", named, MiB, HTABLE, "", max_len, route) == route


@pytest.mark.gpu
@every_lean_route
def test_lean_interior_stream_longer_than_the_hint(cuda, lean):
    """A stream of max_len + 1 bytes among interior ones, in the middle of its wave: EZ_EINVAL,
    size 0, its slot untouched; its wave never enters the interior loop and its neighbours are
    the oracle's."""
    import eazy_amd as ez

    route, max_len, G, CAP = lean
    bufs = tuple(_log_planted(400 + k, n) for k, n in enumerate((3000, 4096, max_len + 1, 2000, 500, 4095, 100, 1500, 700)))
    dev = DevBatch(cuda, bufs)
    got, cb = run_k1(dev, max_len, HTABLE, out=dev.guarded())
    assert got == route
    good = [s for s in range(len(bufs)) if s != 2]
    want = [None] * len(bufs)
    for s, w in zip(good, oracle_of(tuple(bufs[s] for s in good), HTABLE)):
        want[s] = w
    check_refusals(cb, want, f"max_len + 1 on {route}", (2,), ez.EINVAL)
