"""k1_lean's window after the VALU trim (ez_k1_lean.hip, lean_run): the record built as two
dwords (rec_pack32: lo = lit | len << 20, hi = len >> 12 | dist << 8 | force << 28), the
acceptance and the loop tests formed from lane masks on the scalar side, the hand-over of the
first acceptor's next position, and the two exits of the interior loop.

A wrong record field or a hand-over from the wrong lane still writes a stream that decodes back
to something; only its bytes differ from Go's.  So every batch is compared byte for byte with
the C oracle (run_route's bar), on inputs built by hand with k1_inputs' builders, and the CPU
tests first read the oracle's own tokens (k1_inputs.tokens_of, pyoracle's decoder) and
pyoracle's trace of accepts and assert that each stream holds the field value, the acceptor
lane or the window it was built for: a test cannot pass by missing its case.

The record area cannot be filled by an accepted stream (every record moves `done` on by at least
6 bytes and the area holds max_len / 6 + 1 records; test_gpu_k1_lean_interior.py has the
argument), so the loop test's record-room term is exercised by the densest stream the builders
give, one record per 8 bytes with max_len equal to the length, next to the exit by position.

The GPU tests are marked one by one: the tests of the inputs run on the CPU."""

import functools

import numpy as np
import pytest

import k1_inputs as ki
import oracle as orc
from test_gpu_k1_edges import run_route
from test_gpu_k1_hints import _log_planted

MiB = 1 << 20
HTABLE = 1024

# (route, max_len, G, CAP): launch_lean's choices; the 8-lane routes at their largest hints, so
# the streams reach n = 16,384 and n = 65,536
LEAN = [("s:lean g16 fw40", 4096, 16, 40), ("s:lean g8 fw40", 16384, 8, 40), ("s:lean g8 fw24", 65536, 8, 24)]
LEAN_IDS = [r[0].replace(" ", "-") for r in LEAN]
every_lean_route = pytest.mark.parametrize("lean", LEAN, ids=LEAN_IDS)


def windows_of(trace, G):
    """[(iteration, lane, event)] of a stream's accepts: the wave iteration (window count from 0)
    in which lean_run accepts each of Go's matches and the accepting lane.  A window at i judges
    i .. i + G - 1 and moves to i + G when none accepts, to the match's end when one does."""
    out, i, it = [], 0, 0
    for ev in trace:
        if ev[0] in ("far", "short"):
            continue
        x = ev[1]
        while x >= i + G:
            i += G
            it += 1
        out.append((it, x - i, ev))
        i = ev[4]
        it += 1
    return out


# ------------------------------------------------------------------ record fields


def long_run(b, R, tail, lead=64):
    """`lead` filler bytes, then one byte R + 1 times: a run of R bytes at distance 1."""
    b.fill(lead)
    u = b.fill(1, avoid=(b.d[-1],))
    x = b.copy(u, R)
    b.accept("runlen", x, u, x, x + R)
    b.fill(tail)


def long_zeros(b, Z, tail):
    b.fill(21)
    z = b.raw(bytes(Z))
    b.accept("zeros", z + 1, z, z, z + Z)
    b.fill(tail)


def far_copy(b, dist, window, n):
    """A 12-byte marker early and once more `dist` bytes on in filler; no position between has
    the hash of the marker's first four bytes (k1_inputs.keep_bucket_free), so its table entry
    lasts.  window: an anchor copy moves done past the marker first (force stays 0)."""
    b.events = None
    b.fill(30)
    s = b.fill(12)
    if window:
        b.anchor(4, pend=9)
    x = s + dist
    b.fill(x - b.pos())
    ki.keep_bucket_free(b, s, x)
    at = b.copy(s, 12)
    b.accept("window" if window else "runlen", at, s, at, at + 12, must=True)
    b.fill(n - b.pos())


def ends_with_run(b, n, R):
    """n bytes that end with a run of R bytes of period 3: the match's nx is n."""
    b.fill(n - R - 3)
    u = b.fill(3, avoid=(b.d[-1],))
    x = b.copy(u, R)
    b.accept("runlen", x, u, x, x + R)
    assert b.pos() == n


def ends_with_copy(b, n, L):
    """n bytes that end with a window match of L bytes (k1_inputs.fwd after a prefix)."""
    b.fill(n - 2 * L - 29)
    ki.fwd(b, L, 0, 0)
    assert b.pos() == n


@functools.lru_cache(maxsize=None)
def field_cases(max_len, G, CAP):
    seed = [21000 + 100 * G + CAP]

    def mk(name, fn):
        seed[0] += 1
        return ki.make(f"{name} (G {G}, cap {CAP})", fn, seed[0], htable=HTABLE)

    cases = []
    if max_len == 4096:
        # the same shape in a 4 KiB stream: the run to the stream's end, and 20 bytes short of it
        runs = [(4096 - 65, 0), (4000, 11)]
        dists = [(3000, True), (3900, False)]
    else:
        runs = [(4095, 9), (4096, 9), (4097, 9), (4097, 0)]
        dists = [(4096, True), (4100, False), (5000, True)]
    if max_len == 65536:
        runs += [((1 << 16) - 65, 0, 64), ((1 << 16) - 64, 9, 40), ((1 << 16) - 63, 9, 40)]
        dists += [(32768, True), (33001, False), (60000, True)]
    for R, tail, *lead in runs:
        cases.append(mk(f"run of {R} tail {tail}", lambda b, R=R, tail=tail, lead=lead: long_run(b, R, tail, *lead)))
    for Z in (200,) if max_len == 4096 else (200, 4095, 4096, 4097):
        cases.append(mk(f"{Z} zeros", lambda b, Z=Z: long_zeros(b, Z, 12)))
    cases.append(mk("empty forced literal", ki.empty_literal))
    for dist, window in dists:
        n = min(max_len, dist + 200)
        cases.append(mk(f"distance {dist} {'window' if window else 'runlen'}", lambda b, dist=dist, window=window, n=n: far_copy(b, dist, window, n)))
    n = max_len
    cases.append(mk(f"run to the end of {n}", lambda b, n=n: ends_with_run(b, n, 100)))
    cases.append(mk(f"copy to the end of {n}", lambda b, n=n: ends_with_copy(b, n, 50)))
    return tuple(cases)


@every_lean_route
def test_field_inputs_are_what_they_claim(lean):
    """CPU.  Every listed field value is in the oracle's tokens of the committed seed."""
    _, max_len, G, CAP = lean
    cases = field_cases(max_len, G, CAP)
    toks = {}
    for c in cases:
        comp = orc.compress(MiB, HTABLE, [c.data])
        toks[c.name] = ki.tokens_of(comp)[0]
        assert toks[c.name] == c.tokens and 4 <= len(c.data) <= max_len, c.name
    copies = [t for ts in toks.values() for t in ts if t[0] == "c"]
    lens = {t[1] for t in copies}
    zlens = {t[1] for t in copies if t[2] == 0}
    dists = {t[2] for t in copies}
    assert 200 in zlens  # a zero-run record (dist 0)
    assert any(("l", 0) in ts for ts in toks.values())  # the forced empty literal
    if max_len == 4096:
        assert {4031, 4000} <= lens and {3000, 3900} <= dists
    else:
        assert {4095, 4096, 4097} <= lens and {4095, 4096, 4097} <= zlens
        assert {4096, 4100, 5000} <= dists
    if max_len == 65536:
        assert {65471, 65472, 65473} <= lens and {32768, 33001, 60000} <= dists
    # nx at the stream's end, at the route's longest stream
    for c in cases:
        if "to the end" in c.name:
            ev = [e for e in c.trace if e[0] not in ("far", "short")][-1]
            assert len(c.data) == max_len and ev[4] == max_len, c.name
        if c.name.startswith("run of") and c.name.split(" (")[0].endswith("tail 0"):
            assert c.trace[-1][4] == len(c.data), c.name


@pytest.mark.gpu
@every_lean_route
def test_lean_record_fields(cuda, lean):
    """Lengths, distances, zero runs and the force bit on both sides of the record's dword seam,
    each stream twice (side by side and beside the next case)."""
    route, max_len, G, CAP = lean
    named = [(f"{c.name} #{k}", c.data) for c in field_cases(max_len, G, CAP) for k in range(2)]
    assert run_route(cuda, "record fields", named, MiB, HTABLE, "", max_len, route) == route


# ------------------------------------------------------------------ the hand-over


def padded(fn, pad):
    def f(b):
        b.fill(pad)
        fn(b)

    return f


def ext_fn(kind, CAP, lane):
    """A stream whose last match has a count at its cap: forward, backward, or both."""
    if kind == "forward":
        return lambda b: ki.fwd(b, CAP + 30, lane, 40)
    if kind == "backward":
        return lambda b: (ki.back(b, 9, 3, False), b.fill(40))
    return lambda b: (ki.back(b, 9, 3, False, F=CAP + 10), b.fill(40))


def target_of(case):
    """The accept a hand-over case is about: the 12-byte copy of a `restore` stream (its second
    accept), the last accept of a stream with a capped count."""
    acc = [e for e in case.trace if e[0] not in ("far", "short")]
    return acc[1] if case.name.startswith("lane") else acc[-1]


@functools.lru_cache(maxsize=None)
def handover_waves(G, CAP):
    """[(kind, [Case] * (64 / G))]: per kind of capped count one wave of streams whose target
    accepts fall into the same wave iteration at different lanes: the stream with the capped
    count second, the others `restore` streams (the acceptor's i + 1 insert decides their next
    copy's distance).  Streams are brought into step by G filler bytes per missing window."""
    S = 64 // G
    waves = []
    for w, kind in enumerate(("forward", "backward", "both")):
        fns = []
        for k in range(S):
            lane = (5 * w + 3 * k) % G
            fns.append((f"{kind} cap, lane {lane}", ext_fn(kind, CAP, lane)) if k == 1 else (f"lane {lane} k 1", lambda b, lane=lane: ki.restore(b, 1, lane)))
        seeds = [22000 + 1000 * w + 40 * G + CAP + k for k in range(S)]
        first = [ki.make(f"{name} (G {G}, cap {CAP})", fn, sd, htable=HTABLE) for (name, fn), sd in zip(fns, seeds)]
        its = [next(it for it, _, ev in windows_of(c.trace, G) if ev == target_of(c)) for c in first]
        cases = [c if it == max(its) else ki.make(c.name, padded(fn, (max(its) - it) * G), sd + 20, htable=HTABLE)
                 for c, it, (_, fn), sd in zip(first, its, fns, seeds)]
        waves.append((kind, cases))
    return tuple(waves)


@functools.lru_cache(maxsize=None)
def lane_cases(G, CAP):
    """Per lane 0 .. G - 1 two `restore` streams: the later copy finds the acceptor's i + 1
    insert (k = 1) or an entry that a lane past the acceptor had to put back (k = 2)."""
    return tuple(ki.make(f"lane {lane} k {k} (G {G}, cap {CAP})", lambda b, lane=lane, k=k: ki.restore(b, k, lane), 23000 + 40 * G + 2 * lane + k, htable=HTABLE)
                 for lane in range(G) for k in (1, 2))


@every_lean_route
def test_handover_inputs_are_what_they_claim(lean):
    """CPU.  Every lane of a group is the first acceptor of a window whose next copy depends on
    the hand-over; the waves hold one capped count beside accepts at other lanes in one iteration."""
    _, max_len, G, CAP = lean
    seen = set()
    for c in lane_cases(G, CAP):
        comp = orc.compress(MiB, HTABLE, [c.data])
        assert ki.tokens_of(comp)[0] == c.tokens, c.name
        k = int(c.name.split()[3])
        (_, lane, ev), (_, _, nxt) = [w for w in windows_of(c.trace, G)][1:3]
        assert lane == int(c.name.split()[1]) and ev[4] - ev[3] == 12, c.name
        assert nxt[2] == (ev[1] if k < 2 else ev[2]) + k, c.name  # found at the copy (i, i + 1) or at its source
        seen.add(lane)
    assert seen == set(range(G))
    assert ki.tokens_of(orc.compress(MiB, HTABLE, [no_accept(G)]))[0] == [("l", 300)]
    for kind, cases in handover_waves(G, CAP):
        assert len(cases) == 64 // G
        at = []
        for c in cases:
            assert ki.tokens_of(orc.compress(MiB, HTABLE, [c.data]))[0] == c.tokens, c.name
            at.append(next((it, lane) for it, lane, ev in windows_of(c.trace, G) if ev == target_of(c)))
        assert len({it for it, _ in at}) == 1 and len({lane for _, lane in at}) >= min(4, G // 2), (kind, at)
        _, x, _, ist, iend = target_of(cases[1])
        assert (iend - x > CAP) == (kind != "backward") and (x - ist > 8) == (kind != "forward"), (kind, x, ist, iend)
        for c in cases[:1] + cases[2:]:
            _, x, _, ist, iend = target_of(c)
            assert iend - x < CAP and x - ist < 8, c.name


def no_accept(G):
    return np.random.default_rng(24000 + G).integers(1, 256, 300, dtype=np.uint8).tobytes()


@pytest.mark.gpu
@every_lean_route
def test_lean_handover(cuda, lean):
    """The waves with one capped count first (each a whole wave), then every acceptor lane, a
    stream without an accept, and the capped streams once more among other neighbours."""
    route, max_len, G, CAP = lean
    named = [(f"{kind} wave: {c.name}", c.data) for kind, cases in handover_waves(G, CAP) for c in cases]
    assert len(named) % (64 // G) == 0
    named += [(c.name, c.data) for c in lane_cases(G, CAP)]
    named.append(("no accept", no_accept(G)))
    named += [(f"{kind} again: {cases[1].name}", cases[1].data) for kind, cases in handover_waves(G, CAP)]
    assert run_route(cuda, "hand-over", named, MiB, HTABLE, "", max_len, route) == route


# ------------------------------------------------------------------ interior <-> general


def dense_runs(b, n):
    """A record per 8 bytes: two bytes and 6 more of their period, every pair once (a four-byte
    gram seen before would be found as a window match of 8), up to n bytes."""
    b.events = None
    k = 0
    while b.pos() + 8 + 4 <= n:
        u = b.raw(bytes((1 + k % 127, 128 + (3 * (k // 127) + k) % 128)))
        x = b.copy(u, 6)
        b.accept("runlen", x, u, x, x + 6)
        k += 1
    assert k < 64 * 127
    b.fill(n - b.pos())


@functools.lru_cache(maxsize=None)
def dense_case(n):
    return ki.make(f"a record per 8 bytes, {n} bytes", lambda b: dense_runs(b, n), 25000 + n % 64, htable=HTABLE)


# the dense stream's length per route: the hint is the length itself (any value of the route's range)
DENSE_N = {4096: 4096, 16384: 6000, 65536: 16500}


@every_lean_route
def test_exit_inputs_are_what_they_claim(lean):
    """CPU.  The dense stream has a record per 8 bytes: (n - 4) // 8 copies against a record area
    of n // 6 + 1."""
    _, max_len, G, CAP = lean
    n = DENSE_N[max_len]
    c = dense_case(n)
    toks = ki.tokens_of(orc.compress(MiB, HTABLE, [c.data]))[0]
    assert len(c.data) == n and toks == c.tokens
    assert sum(t[0] == "c" for t in toks) == (n - 4) // 8 < n // 6 + 1


@pytest.mark.gpu
@every_lean_route
def test_lean_one_stream_ends_60_bytes_early(cuda, lean):
    """Whole waves of equal streams but one, 60 bytes shorter, at each place of its wave: the wave
    leaves the interior loop for that stream while the others still have interior windows."""
    route, max_len, G, CAP = lean
    S = 64 // G
    n = min(max_len, 8192)
    full = _log_planted(500 + G + CAP, n)
    named = []
    for at in range(S):
        named += [(f"wave {at}: {'60 bytes short' if k == at else 'full'}", full[: n - 60] if k == at else full) for k in range(S)]
    assert run_route(cuda, "one stream 60 bytes short", named, MiB, HTABLE, "", max_len, route) == route


@pytest.mark.gpu
@every_lean_route
def test_lean_dense_records_at_the_hint(cuda, lean):
    """max_len equal to the length and a record per 8 bytes: a wave of such streams, and one
    among sparse streams of the same length."""
    route, max_len, G, CAP = lean
    S = 64 // G
    n = DENSE_N[max_len]
    c = dense_case(n)
    rng = np.random.default_rng(26000 + n)
    named = [(f"dense #{k}", c.data) for k in range(S)]
    named += [("dense among sparse", c.data)] + [(f"random {n} #{k}", rng.integers(1, 256, n, dtype=np.uint8).tobytes()) for k in range(S - 2)]
    named.append(("logs", _log_planted(600 + G, n)))
    assert run_route(cuda, "dense records", named, MiB, HTABLE, "", n, route) == route
