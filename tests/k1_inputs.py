"""Inputs for K1 (the encoder) whose parse by Go is known before the oracle runs.

TEST INFRASTRUCTURE ONLY.  Every case is one single-Write stream built byte by byte so that
it sits on one of K1's structural edges (DESIGN §4 has the table), together with what Go's
Writer must make of it:

  tokens  the stream's token list, ("l", n) per literal and ("c", n, distance) per copy
          (distance 0: the zero token), in order;
  events  pyoracle's trace of accepted matches, (branch, i, candidate, ist, iend) with
          positions in the stream -- where Go accepted, how far it found backward (i - ist)
          and forward (iend - i);
  far     positions at which Go must skip a candidate more than a block back.

Filler is seeded random bytes in 1..255, so an accidental 6-byte match is out of the question
and no zero byte occurs by chance.  A planted copy has the byte before it and the byte after
it forced to differ from the source's neighbours.  What cannot be forced (a table bucket
overwritten by a colliding position in between, mostly) is left to a seed search: a builder is
tried with up to SEEDS seeds until the C oracle's tokens and pyoracle's trace are the intended
ones, and raises when it runs out.  The search runs on the CPU against the oracles only."""

from __future__ import annotations

import functools

import numpy as np

import oracle as orc
import pyoracle as po

MiB = 1 << 20
KiB = 1 << 10
SEEDS = 64


class Retry(Exception):
    """This seed's bytes do not allow the construction (a forced-different byte is equal)."""


class Unbuildable(AssertionError):
    pass


# ------------------------------------------------------------------ tokens of a stream


def tokens_of(comp: bytes):
    """The token list of a compressed stream (metas skipped) and each token's offset in it."""
    toks, at = [], []
    i = 0
    while i < len(comp):
        tag, l, j, err = po.dec_tag(comp, i)
        assert err == 0, (i, err)
        if tag == po.META and l == 0:
            _, ml, j, err = po.dec_meta(comp, j)
            assert err == 0
            i = j + ml
            continue
        at.append(i)
        if tag == po.LITERAL:
            toks.append(("l", l))
            i = j + l
        else:
            off, j, err = po.dec_offset(comp, j, l)
            assert err == 0
            toks.append(("c", l, off))
            i = j
    return toks, at


def token_at(comp: bytes, byte: int) -> str:
    """'token k = (...)' for the token that holds offset `byte` of the compressed stream."""
    toks, at = tokens_of(comp)
    k = -1
    for k in range(len(at) - 1, -1, -1):
        if at[k] <= byte:
            break
    return "header" if k < 0 or byte < at[0] else f"token {k} = {toks[k]} at byte {at[k]}"


def gram_hash(g: bytes, htable: int) -> int:
    """writer.go:491-493 for a table of `htable` entries."""
    hsh = 32 - (htable - 1).bit_length()
    return ((int.from_bytes(g[:4], "little") * 0x1E35A7BD) & 0xFFFFFFFF) >> hsh


# ------------------------------------------------------------------ the byte builder


class Build:
    """A stream under construction and the parse it is meant to have."""

    def __init__(self, seed: int, htable: int = 1024):
        self.rng = np.random.default_rng(seed)
        self.htable = htable
        self.d = bytearray()
        self.avoid = None  # the next appended byte must differ from this one
        self.done = 0
        self.toks = []
        self.events = []  # None: the trace's accepts are not all checked, only those in must
        self.must = []
        self.far = []
        self.short = []  # (i, candidate) that Go must look at in the block and refuse as too short

    # bytes ---------------------------------------------------------------
    def pos(self) -> int:
        return len(self.d)

    def _first(self, b: int) -> None:
        if self.avoid is not None and b == self.avoid:
            raise Retry
        self.avoid = None

    def fill(self, k: int, avoid=()) -> int:
        """k filler bytes; -> where they start."""
        at = len(self.d)
        assert k >= 0, k
        v = self.rng.integers(1, 256, k, dtype=np.uint8)
        for t in range(k if avoid else min(k, 1)):
            while v[t] in avoid or (t == 0 and v[t] == self.avoid):
                v[t] = self.rng.integers(1, 256)
        if k:
            self.avoid = None
        self.d += v.tobytes()
        return at

    def raw(self, bs: bytes) -> int:
        at = len(self.d)
        if bs:
            self._first(bs[0])
            self.d += bs
        return at

    def copy(self, src: int, L: int) -> int:
        """The L bytes at src again (the source may overlap its copy: a run); the byte before
        must differ from the source's, the byte appended next will."""
        at = len(self.d)
        if L == 0:
            return at
        if src > 0 and at > 0 and self.d[at - 1] == self.d[src - 1]:
            raise Retry
        self._first(self.d[src])
        for t in range(L):
            self.d.append(self.d[src + t])
        self.avoid = self.d[src + L]
        return at

    def collider(self, gram: bytes) -> bytes:
        """Four filler bytes, not `gram`, with gram's hash."""
        h = gram_hash(gram, self.htable)
        for _ in range(64):
            c = self.rng.integers(1, 256, (1 << 14, 4), dtype=np.uint32)
            u = c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16 | c[:, 3] << 24
            hh = (u * np.uint32(0x1E35A7BD)) >> np.uint32(32 - (self.htable - 1).bit_length())
            for k in np.nonzero(hh == h)[0]:
                g = bytes(int(v) for v in c[k])
                if g != bytes(gram[:4]):
                    return g
        raise Retry

    # the intended parse --------------------------------------------------
    def accept(self, branch: str, i: int, cand: int, ist: int, iend: int, dist=None, must=False) -> None:
        """Go accepts at i the candidate cand and emits the copy [ist, iend)."""
        if must:
            self.must.append((branch, i, cand, ist, iend))
        if branch == "cut":
            self.toks.append(("l", iend - ist))
        else:
            if self.done < ist or branch == "runlen":
                self.toks.append(("l", ist - self.done))
            self.toks.append(("c", iend - ist, 0 if branch == "zeros" else (i - cand if dist is None else dist)))
        if self.events is not None:
            self.events.append((branch, i, cand, ist, iend))
        self.done = iend

    def anchor(self, src: int, pend: int = 0, L: int = 8) -> int:
        """`pend` filler bytes and a copy of L bytes from src, found at its first byte:
        moves done to here.  -> the copy's position."""
        self.fill(pend)
        at = self.copy(src, L)
        self.accept("window" if src + L <= self.done else "runlen", at, src, at, at + L)
        return at

    def finish(self):
        if self.done < len(self.d):
            self.toks.append(("l", len(self.d) - self.done))
        return bytes(self.d)


class Case:
    """A built stream: name, data, block, htable, the intended tokens / events / far skips,
    and what the two oracles made of it (comp: the C oracle's bytes; py_comp, trace: pyoracle's)."""

    def __init__(self, name, data, block, htable, toks, events, far, short, comp, py_comp, trace, seed):
        self.name, self.data, self.block, self.htable = name, data, block, htable
        self.tokens, self.events, self.far, self.short, self.must = toks, events, far, short, ()
        self.comp, self.py_comp, self.trace, self.seed = comp, py_comp, trace, seed

    def __repr__(self):
        return f"Case({self.name}, {len(self.data)} bytes, seed {self.seed})"


def py_parse(data: bytes, block: int, htable: int):
    w = po.Writer(block, htable)
    w.trace = []
    n, err = w.write(data)
    assert err == 0 and n == len(data)
    return w.sink, w.trace


def verdict(b: Build, data: bytes, block: int, htable: int):
    """-> (comp, py_comp, trace, None) when both oracles give the intended parse, else a
    reason in the last place."""
    comp = orc.compress(block, htable, [data])
    got = tokens_of(comp)[0]
    if got != b.toks:
        return comp, None, None, f"tokens {got[:12]} ..., intended {b.toks[:12]} ..."
    py_comp, trace = py_parse(data, block, htable)
    acc = [e for e in trace if e[0] not in ("far", "short")]
    if b.events is not None and acc != b.events:
        return comp, py_comp, trace, f"trace {acc[:8]} ..., intended {b.events[:8]} ..."
    if not set(b.must) <= set(acc):
        return comp, py_comp, trace, f"trace lacks {[e for e in b.must if e not in acc]}"
    fars = {e[1] for e in trace if e[0] == "far"}
    if not set(b.far) <= fars:
        return comp, py_comp, trace, f"far skips lack {b.far}"
    shorts = {e[1:] for e in trace if e[0] == "short"}
    if not set(b.short) <= shorts:
        return comp, py_comp, trace, f"refused candidates lack {b.short}"
    return comp, py_comp, trace, None


def make(name: str, fn, seed: int, block: int = MiB, htable: int = 0) -> Case:
    """fn(Build) lays the bytes and the intended parse down; the first of SEEDS seeds whose
    stream both oracles parse as intended is the case."""
    htable = htable or (4096 if block == 4096 else 1024)  # a source a block back has to last in the table
    why = "every seed refused by the builder"
    for s in range(seed * SEEDS, (seed + 1) * SEEDS):
        b = Build(s, htable)
        try:
            fn(b)
        except Retry:
            continue
        data = b.finish()
        comp, py_comp, trace, why = verdict(b, data, block, htable)
        if why is None:
            case = Case(name, data, block, htable, b.toks, b.events, b.far, b.short, comp, py_comp, trace, s)
            case.must = tuple(b.must)
            return case
    raise Unbuildable(f"{name}: no seed of {SEEDS} gives the intended parse; the last: {why}")


# ------------------------------------------------------------------ A: forward counts

A_LANE_L = (6, 23, 24, 25, 39, 40, 41, 88, 89, 104, 105, 152, 153, 168, 169)


def fwd(b: Build, L: int, lane: int, tail: int = 11):
    """A source of L bytes, an anchor copy that moves done past it, `lane` filler bytes and
    the L bytes again: a window match found at its first byte, nothing backward, L forward."""
    b.fill(2)
    src = b.fill(L)
    asrc = b.fill(14) + 3
    b.anchor(asrc, pend=5)
    b.fill(lane)
    x = b.copy(src, L)
    if L >= 6:
        b.accept("window", x, src, x, x + L)
    b.fill(tail)


def group_a():
    cases = [make(f"A-len{L}", lambda b, L=L: fwd(b, L, 3), 1000 + L) for L in list(range(5, 301)) + [379, 380, 381]]
    for lane in range(17):
        for L in A_LANE_L:
            cases.append(make(f"A-lane{lane}-len{L}", lambda b, L=L, lane=lane: fwd(b, L, lane), 2000 + 32 * lane + L % 32))
    return cases


# ------------------------------------------------------------------ B: backward counts

B_FREE = tuple(range(41)) + (71, 72, 73, 135, 136, 137)
B_BOUND = ((0, 0), (1, 0), (7, 0), (8, 0), (9, 0), (5, 2), (8, 3), (23, 1), (24, 0), (40, 3),(72, 0), (136, 1))


def back(b: Build, B: int, P: int, bounded: bool, F: int = 8):
    """Go's first successful lookup inside the plant is B bytes into it and extends B bytes
    backward: the plant is T[8:] + V[:F], T the target of an earlier copy of B + 8 bytes from
    U (positions inside a copy are not in the table), V the fresh bytes after T, and U's own
    table entries are overwritten, one 'U's 4-gram plus a differing byte' item per position.
    Free: P filler bytes before the plant, the last one differing.  Bounded: the P bytes
    before the plant and the copy that ends before them continue T backward, so only done
    stops the count (B + P bytes found backward)."""
    asrc = b.fill(12) + 2
    u = b.fill(B + 8)
    if bounded:
        b.fill(3)
        w = b.fill(4)
        b.raw(bytes(b.d[u + 4 - P : u + 8 - P]))
        b.avoid = b.d[u + 8 - P]
    b.fill(6)
    t = b.copy(u, B + 8)
    b.accept("runlen", t, u, t, t + B + 8)
    v = b.fill(F + 4)
    for k in range(0 if bounded else 4, B + 5):
        b.raw(bytes(b.d[u + k : u + k + 4]))
        b.fill(1, avoid=(b.d[u + k + 4], b.d[u + k]))
    b.fill(2)
    if bounded:
        b.anchor(w, pend=2)
        b.raw(bytes(b.d[t + 8 - P : t + 8]))
    else:
        b.anchor(asrc, pend=2)
        b.fill(P, avoid=(b.d[t + 7],))
    x = b.raw(bytes(b.d[t + 8 : t + 8 + B]) + bytes(b.d[v : v + F]))
    b.avoid = b.d[v + F]
    b.accept("window", x + B, v, b.done if bounded else x, x + B + F)
    b.fill(10)


def group_b():
    cases = [make(f"B-back{B}", lambda b, B=B: back(b, B, 3, False), 3000 + B) for B in B_FREE]
    cases += [make(f"B-back{B}-done-after{P}", lambda b, B=B, P=P: back(b, B, P, True), 3200 + B + P) for B, P in B_BOUND]
    return cases


# ------------------------------------------------------------------ C: window mechanics


def restore(b: Build, k: int, lane: int):
    """A copy of 12 bytes of A accepted at x; later A[k:k+7] again.  Go inserted x and x + 1
    only, so k = 0, 1 find the copy (x + k) and k >= 2 must still find A + k: the entry that a
    lane after the acceptor touched."""
    a = b.fill(24) + 4
    asrc = b.fill(12) + 2
    b.anchor(asrc, pend=4)
    b.fill(lane)
    x = b.copy(a, 12)
    b.accept("window", x, a, x, x + 12)
    b.fill(7)
    y = b.copy(a + k, 7)
    b.accept("window", y, (x if k < 2 else a) + k, y, y + 7)
    b.fill(9)


def evict(b: Build, kill: int, lane: int):
    """A source of 6 bytes has 3 four-grams.  `kill` of them (the first ones) are overwritten by
    colliding four-grams laid down in the window of the plant, before it.  kill = 3: Go finds
    no copy.  kill = 1, 2: Go accepts at the plant's byte `kill` and finds `kill` bytes backward."""
    a = b.fill(16) + 5
    asrc = b.fill(12) + 2
    b.anchor(asrc, pend=4)
    b.fill(lane)
    for k in range(kill):
        b.raw(b.collider(bytes(b.d[a + k : a + k + 4])))
    b.fill(1)
    x = b.copy(a, 6)
    if kill < 3:
        b.accept("window", x + kill, a + kill, x, x + 6)
    b.fill(9)


def keep_after(b: Build, lane: int):
    """A[4:8] has the hash of E[0:4], E's other four-grams are overwritten.  A copy of 10 bytes
    of A is accepted at x: position x + 4 lies inside it and is not inserted, so E's entry
    stands and the 6 bytes of E are found afterwards."""
    a = b.fill(4)
    hole = b.fill(4)
    b.fill(4)
    e = b.fill(6)
    b.d[hole : hole + 4] = b.collider(bytes(b.d[e : e + 4]))
    b.fill(3)
    for k in (1, 2):
        b.raw(b.collider(bytes(b.d[e + k : e + k + 4])))
        b.fill(1)
    asrc = b.fill(12) + 2
    b.anchor(asrc, pend=4)
    b.fill(lane)
    x = b.copy(a, 10)
    b.accept("window", x, a, x, x + 10)
    b.fill(3)
    y = b.copy(e, 6)
    b.accept("window", y, e, y, y + 6)
    b.fill(9)


def at_end(b: Build, L: int, window: bool):
    """A copy of L bytes that ends with the stream: L = 6 is the last position Go looks at."""
    src = b.fill(16) + 3
    asrc = b.fill(12) + 2
    if window:
        b.anchor(asrc, pend=4)
    b.fill(3)
    x = b.copy(src, L)
    if L >= 6:
        b.accept("window" if window else "runlen", x, src, x, x + L)


def tiny(b: Build, n: int):
    """n bytes of period 3: one copy from n = 9 on (candidate 0, the empty entry's twin)."""
    b.fill(3)
    b.copy(0, n - 3)
    if n >= 9:
        b.accept("runlen", 3, 0, 3, n)


def group_c():
    cases = []
    for k in range(7):
        cases.append(make(f"C-restore-k{k}", lambda b, k=k: restore(b, k, 2 + k), 4000 + k))
    for kill in (1, 2, 3):
        for lane in (0, 3):
            cases.append(make(f"C-evict{kill}-lane{lane}", lambda b, kill=kill, lane=lane: evict(b, kill, lane), 4010 + 4 * kill + lane))
    for lane in (0, 1, 5, 9):
        cases.append(make(f"C-keep-after-lane{lane}", lambda b, lane=lane: keep_after(b, lane), 4030 + lane))
    for L in (4, 5, 6, 7, 30):
        for window in (False, True):
            cases.append(make(f"C-end-len{L}-{'window' if window else 'runlen'}", lambda b, L=L, window=window: at_end(b, L, window), 4040 + 2 * L + window))
    for n in range(4, 20):
        cases.append(make(f"C-tiny{n}", lambda b, n=n: tiny(b, n), 4100 + n))
    return cases


# ------------------------------------------------------------------ D: position 0 and before


def head_repeat(b: Build, L: int):
    """The stream's first L bytes again while done == 0: candidate 0 in the pending literal,
    the runlen branch, nothing before the stream."""
    b.fill(L + 9)
    b.fill(7)
    x = b.copy(0, L)
    b.accept("runlen", x, 0, x, x + L)
    b.fill(9)


def head_after_zeros(b: Build, k: int, L: int):
    """After an earlier copy, k zero bytes and the stream's first L bytes: candidate 0 in the
    block, and the block's bytes before position 0 are zero, so up to 6 zero bytes are found
    backward before the stream's first byte.  7 zeros are a period-1 run of 6 first, 8 the zero
    token."""
    b.fill(L + 9)
    asrc = b.fill(12) + 2
    b.anchor(asrc, pend=4)
    b.fill(3)
    z = b.raw(bytes(k))
    y = b.raw(bytes(b.d[0:L]))
    b.avoid = b.d[L]
    if k <= 6:
        b.accept("window", y, 0, y - k, y + L, dist=y)
    elif k == 7:
        b.accept("runlen", z + 1, z, z + 1, y)
        b.accept("window", y, 0, y, y + L)
    else:
        b.accept("zeros", z + 1, z, z, y)
        b.accept("window", y, 0, y, y + L)
    b.fill(9)


def near_head_after_zeros(b: Build, c: int, k: int, L: int = 13):
    """The same with the table entries of the stream's first c four-grams overwritten: Go accepts
    c bytes into the plant with candidate c (1..7: the candidate's 8 bytes backward reach before
    the stream) and finds c bytes of the stream and k zero bytes of the empty block backward."""
    b.fill(L + 9)
    for j in range(c):
        b.raw(b.collider(bytes(b.d[j : j + 4])))
        b.fill(1)
    asrc = b.fill(12) + 2
    b.anchor(asrc, pend=4)
    b.fill(3)
    b.raw(bytes(k))
    y = b.raw(bytes(b.d[0:L]))
    b.avoid = b.d[L]
    b.accept("window", y + c, c, y - k, y + L)
    b.fill(9)


def group_d():
    cases = [make(f"D-head-len{L}", lambda b, L=L: head_repeat(b, L), 5000 + L) for L in (6, 24, 41)]
    for k in range(1, 9):
        cases.append(make(f"D-head-after-{k}-zeros", lambda b, k=k: head_after_zeros(b, k, 13), 5100 + k))
    for c, k in ((1, 3), (4, 2), (7, 1), (7, 5)):
        cases.append(make(f"D-candidate-{c}-after-{k}-zeros", lambda b, c=c, k=k: near_head_after_zeros(b, c, k), 5200 + 8 * c + k))
    return cases


def before_of(case: Case) -> bytes:
    """The 8 bytes in front of the case's last accepted copy: a preceding stream that ends in
    them would extend that copy backward if a kernel read before its own stream."""
    ist = case.events[-1][3]
    return bytes(case.data[max(0, ist - 8) : ist]).rjust(8, b"\x07")


# ------------------------------------------------------------------ E: runs and zeros


def run(b: Build, per: int, R: int, anchored: bool):
    """A unit of `per` fresh bytes, then R more bytes of the same period."""
    asrc = b.fill(12) + 2
    if anchored:
        b.anchor(asrc, pend=4)
    b.fill(7)
    u = b.fill(per)
    x = b.copy(u, R)
    if R >= 6:
        b.accept("runlen", x, u, x, x + R)
    b.fill(9)


def run_again(b: Build, per: int):
    """A run of 24 bytes of period `per`, accepted at its unit's second occurrence x with
    candidate x - per.  The lane `per` positions after the acceptor has the acceptor's four-gram
    and the acceptor's position as its candidate, and Go never visits it: 8 bytes of the run
    again are found at x (Go's entry), not at x + per."""
    b.fill(7)
    u = b.fill(per)
    x = b.copy(u, 24)
    b.accept("runlen", x, u, x, x + 24)
    b.fill(9)
    y = b.copy(x, 8)
    b.accept("window", y, x, y, y + 8)
    b.fill(9)


def zeros(b: Build, Z: int, at_end_: bool):
    """Z zero bytes.  In the middle: the zero token from 8 on, a period-1 run of 6 for 7.  At
    the stream's end st + 8 < n fails for Z = 8: a period-1 run of 7."""
    b.fill(21)
    z = b.raw(bytes(Z))
    token = Z >= (9 if at_end_ else 8)
    if token:
        b.accept("zeros", z + 1, z, z, z + Z)
    elif Z >= 7:
        b.accept("runlen", z + 1, z, z + 1, z + Z)
    if not at_end_:
        b.fill(12)


def zeros_after_copy(b: Build, k: int, Z: int = 12):
    """A copy whose last k bytes are zero, then Z more zeros: the zero token starts at done, the
    k zero bytes before it are not the pending literal's."""
    b.fill(5)
    s = b.fill(6)
    b.raw(bytes(k))
    b.fill(9)
    t = b.copy(s, 6 + k)
    b.accept("runlen", t, s, t, t + 6 + k)
    z = b.raw(bytes(Z))
    b.avoid = None
    b.accept("zeros", z + 1, z, z, z + Z)
    b.fill(9)


def empty_literal(b: Build):
    """writeRunlen emits its literal unconditionally: a run whose backward count reaches done
    gives an empty literal (one 0x00 byte) in front of the copy."""
    a = b.fill(12) + 2
    b.fill(9)
    x = b.anchor(a, pend=5)
    unit = bytes(b.d[x + 4 : x + 8])
    b.avoid = None
    if b.d[a + 8] == unit[0]:
        raise Retry
    b.raw(unit * 3)
    b.avoid = unit[0]
    done = x + 8
    b.accept("runlen", done + 4, done, done, done + 12, dist=4)
    b.fill(9)


def group_e():
    cases = []
    for per in range(1, 10):
        for R in (5, 6, 7, 40, 41, 300):
            cases.append(make(f"E-period{per}-run{R}", lambda b, per=per, R=R: run(b, per, R, False), 6000 + 8 * per + R % 8))
    for per in (1, 4, 9):
        for R in (6, 41):
            cases.append(make(f"E-period{per}-run{R}-after-copy", lambda b, per=per, R=R: run(b, per, R, True), 6100 + 8 * per + R % 8))
    for per in (1, 2, 3, 4, 7, 9):
        cases.append(make(f"E-period{per}-run-again", lambda b, per=per: run_again(b, per), 6150 + per))
    for Z in (5, 6, 7, 8, 9, 24, 25, 40, 41, 200):
        for e in (False, True):
            cases.append(make(f"E-zeros{Z}-{'end' if e else 'middle'}", lambda b, Z=Z, e=e: zeros(b, Z, e), 6200 + 2 * Z + e))
    for k in range(4):
        cases.append(make(f"E-zeros-after-copy-ending-{k}-zeros", lambda b, k=k: zeros_after_copy(b, k), 6700 + k))
    cases.append(make("E-empty-literal", empty_literal, 6800))
    return cases


# ------------------------------------------------------------------ G: the token writer


def literal(b: Build, N: int, first: bool):
    """A literal of exactly N bytes in front of a copy, the stream's first or a later one."""
    if first:
        b.fill(N)
        b.anchor(2)
    else:
        b.fill(20)
        b.anchor(2)
        b.fill(N)
        b.anchor(10)
    b.fill(9)


def distance(b: Build, L: int, dist: int, window: bool):
    """A copy of L bytes at `dist`: the offset field's forms turn on dist - L."""
    s = b.fill(L + 16) + 4
    if window:
        b.anchor(s + L + 2, pend=4)
    b.fill(s + dist - b.pos())
    x = b.copy(s, L)
    b.accept("window" if window else "runlen", x, s, x, x + L)
    b.fill(9)


def records_dict(b: Build, R: int):
    """R copies, each a slice of 6..8 bytes of a 200-byte dictionary at the front with one fresh
    byte in front of it.  A slice's table entry must still stand when it is used, and after a use
    it points at that use: the builder keeps the table of the positions Go inserts (every byte
    of the dictionary, then per copy the fresh byte and the slice's first and second byte) and
    takes the next even dictionary offset whose four-gram the table still leads to."""
    D = 200
    b.fill(D)
    tab = {}

    def ins(p):
        tab[gram_hash(bytes(b.d[p : p + 4]), b.htable)] = p

    for p in range(D - 3):
        ins(p)
    late = list(range(D - 3, D))
    offs = list(range(4, D - 10, 2))
    at = 0
    for r in range(R):
        for _ in offs:
            a = offs[at % len(offs)]
            at += 1
            g = bytes(b.d[a : a + 4])
            p = tab.get(gram_hash(g, b.htable))
            if p is not None and bytes(b.d[p : p + 4]) == g:
                break
        else:
            raise Retry
        L = 6 + a % 3
        u = b.fill(1, avoid=(b.d[p - 1],))
        x = b.raw(bytes(b.d[a : a + L]))
        b.avoid = b.d[p + L]
        b.accept("window" if r else "runlen", x, p, x, x + L)
        for q in late + [u, x, x + 1]:
            ins(q)
        late = []
    b.fill(9)


def records_runs(b: Build, R: int):
    """R copies, each 3 fresh bytes and 6 more of their period: no table entry has to last
    (tokens only: the trace is not held to the acceptors)."""
    for r in range(R):
        u = b.fill(2)
        b.fill(1, avoid=(b.d[u - 1],) if u else ())
        x = b.copy(u, 6)
        b.accept("runlen", x, u, x, x + 6)
    b.events = None  # a record found one byte late (its entry overwritten) has the same tokens
    b.fill(9)


def plain(b: Build, n: int):
    """n bytes with a copy near the front and one that ends 9 bytes before the end."""
    b.fill(40)
    b.anchor(4)
    b.fill(n - b.pos() - 8 - 9 - 1)
    b.anchor(b.pos() - 60, pend=1)
    b.fill(9)
    assert b.pos() == n


G_LIT = (95, 96, 97, 123, 124, 379, 380)


def group_g():
    cases = []
    for N in G_LIT:
        for first in (True, False):
            cases.append(make(f"G-literal{N}-{'first' if first else 'later'}", lambda b, N=N, first=first: literal(b, N, first), 7000 + N % 64 + first))
    for dl in (251, 252, 507, 508):
        for window in (False, True):
            cases.append(make(f"G-dist-len+{dl}-{'window' if window else 'runlen'}", lambda b, dl=dl, window=window: distance(b, 9, 9 + dl, window), 7100 + dl % 64 + window))
    cases.append(make("G-dist-equals-len", lambda b: run(b, 8, 8, False), 7200))
    cases.append(make("G-dist-equals-len-1", lambda b: run(b, 7, 8, False), 7201))
    for R in (318, 319, 320, 321):
        cases.append(make(f"G-records{R}-dictionary", lambda b, R=R: records_dict(b, R), 7300 + R % 8))
        cases.append(make(f"G-records{R}-runs", lambda b, R=R: records_runs(b, R), 7310 + R % 8))
    for n in (4095, 4096):
        cases.append(make(f"G-stream{n}", lambda b, n=n: plain(b, n), 7400 + n % 8))
    return cases


def group_g_long():
    """The cases over 4,096 bytes: kEmitIn's far side and kEwRec's record counts."""
    cases = [make("G-stream4097", lambda b: plain(b, 4097), 7401)]
    for R in (2046, 2047, 2048, 2049):
        cases.append(make(f"G-records{R}-runs", lambda b, R=R: records_runs(b, R), 7500 + R % 8))
    return cases


# ------------------------------------------------------------------ F: placement

F_STARTS = tuple(range(55, 91)) + tuple(range(119, 141))


def at_position(b: Build, x: int, tail: int = 11):
    """A window copy of 12 bytes that starts at stream position x (x >= 55)."""
    src = b.fill(14) + 1
    asrc = b.fill(16) + 3
    b.anchor(asrc, pend=x - 40)
    b.fill(2)
    assert b.pos() == x
    at = b.copy(src, 12)
    b.accept("window", at, src, at, at + 12)
    b.fill(tail)


def group_f():
    cases = [make(f"F-copy-at-{x}", lambda b, x=x: at_position(b, x), 8000 + x) for x in F_STARTS]
    for back_ in range(60, 71):
        cases.append(make(f"F-copy-at-n-{back_}", lambda b, back_=back_: at_position(b, 150, back_ - 12), 8200 + back_))
    return cases


# ------------------------------------------------------------------ H: ring semantics


def ring_distance(b: Build, bs: int, k: int, P: int, L: int = 11):
    """Block bs.  A source at distance bs - k from its plant of L bytes, P pending bytes before
    the plant.  Go trims the copy to the bs - distance = k bytes the ring still holds when the
    copy is written (trim 1), whatever P is: k = 5 no copy, 6 <= k < L a copy of k bytes and
    the rest literal, k >= L the whole plant.  k <= 0 never gives a copy, and done - candidate >
    bs (k + P < 0) is the far skip; every other candidate must be looked at and refused."""
    b.fill((2 * bs if bs <= 1024 else bs) + 50)
    b.anchor(b.pos() - 300)
    s = b.fill(L + 8) + 4
    b.anchor(b.pos() - 200, pend=3)
    x = s + bs - k
    b.fill(x - P - 8 - 5 - b.pos())
    b.anchor(b.pos() - 100, pend=5)
    b.fill(P)
    assert b.pos() == x
    b.copy(s, L)
    if k >= 6:
        b.accept("window", x, s, x, x + min(k, L))
    elif k + P < 0:
        b.far.append(x)
    else:
        b.short.append((x, s))
    b.fill(30)


def ring_cut(b: Build, bs: int, K: int, L: int = 10):
    """Block bs.  A repeat of L bytes at distance K inside one pending literal.  K = bs - 9:
    a copy at distance K.  K >= bs - 8: writeRunlen's cut -- K bytes go out as a literal, the
    parse goes back to their end (5 bytes before the repeat), and the repeat is then found from
    its second byte in the window, one byte backward, trimmed to bs - K bytes."""
    b.fill(40)
    b.anchor(10)
    b.fill(5)
    done = b.done
    st = b.fill(K)
    x = b.copy(st, L)
    assert x - st == K
    if K < bs - 8:
        b.accept("runlen", x, st, x, x + L)
    else:
        b.accept("cut", x, st, done, done + K)
        b.accept("window", x + 1, st + 1, x, x + bs - K)
    b.fill(30)


def ring_far_updates(b: Build, bs: int):
    """Block bs.  S[0:4] + 4 fresh bytes at distance bs + 1 from S with nothing pending: the far
    skip.  Those 8 bytes again right after a later copy: found only if the skipped position went
    into the table: the entries of their other four-grams are overwritten in between."""
    b.fill(bs + 50)
    b.anchor(b.pos() - 300)
    s = b.fill(12) + 4
    b.anchor(b.pos() - 200, pend=3)
    x = s + bs + 1
    b.fill(x - 8 - 5 - b.pos())
    b.anchor(b.pos() - 100, pend=5)
    assert b.pos() == x
    b.raw(bytes(b.d[s : s + 4]))
    b.avoid = b.d[s + 4]
    b.fill(4)
    b.far.append(x)
    b.fill(9)
    for k in range(1, 5):
        b.raw(b.collider(bytes(b.d[x + k : x + k + 4])))
        b.fill(1)
    b.fill(20)
    b.anchor(b.pos() - 30, pend=0)
    y = b.copy(x, 8)
    b.accept("window", y, x, y, y + 8)
    b.fill(30)


def group_h(bs: int):
    cases = []
    for k in (40, 7, 6, 5, 0, -1):
        for P in (0, 1, 30):
            cases.append(make(f"H{bs}-source-at-bs{-k:+d}-pending{P}", lambda b, k=k, P=P: ring_distance(b, bs, k, P), 9000 + 4 * (k + 2) + P % 4 + bs % 7, block=bs))
    for K in (bs - 9, bs - 8, bs - 7):
        cases.append(make(f"H{bs}-repeat-at-bs{K - bs:+d}-in-literal", lambda b, K=K: ring_cut(b, bs, K), 9300 + K % 16, block=bs))
    cases.append(make(f"H{bs}-far-skip-updates-table", lambda b: ring_far_updates(b, bs), 9400 + bs % 7, block=bs))
    return cases


# ------------------------------------------------------------------ I, J: long streams, sparse events

KC_C, KC_W, KC_O = 32768, 8192, 1024  # K1c's chunk, warm-up and overlap for such batches (kc_geom)
KX_C = 16384  # K1x's chunk


def sparse(b: Build, upto: int, lo: int = 300, hi: int = 2000):
    """Filler up to position `upto`, with a copy of 8..20 bytes from 40..250 bytes back (inside
    the pending literal) every lo..hi bytes; the last 60 bytes before `upto` hold no event.
    Such a copy has the same tokens whether its first four-gram's entry still stands or the
    second one's finds it, so only its tokens are held, not its acceptor."""
    b.events = None
    while True:
        gap = int(b.rng.integers(lo, hi))
        if b.pos() + gap + 20 + 60 > upto:
            break
        b.fill(gap)
        back, L = int(b.rng.integers(40, 250)), int(b.rng.integers(8, 21))
        x = b.copy(b.pos() - back, L)
        b.accept("runlen", x, x - back, x, x + L)
    b.fill(upto - b.pos())


def event(b: Build, x: int, L: int = 12, back: int = 100, must: bool = True):
    """Filler up to x and a copy of L bytes from `back` bytes back, in the pending literal."""
    b.fill(x - b.pos())
    at = b.copy(x - back, L)
    b.accept("runlen", at, x - back, at, at + L, must=must)


def k1c_stream(b: Build, kind: str, n: int):
    """n bytes of sparse events; nothing within 600 bytes before chunk 1's start C and 300 past
    C + O but what `kind` names."""
    C, W, O = KC_C, KC_W, KC_O
    src = None
    if kind in ("source-beyond-warmup", "source-within-warmup"):
        sparse(b, C - (W + 500 if kind == "source-beyond-warmup" else 4000))
        src = b.fill(40) + 10
    sparse(b, C - 600)
    if kind == "copy-ends-at-C":
        event(b, C - 12)
    elif kind == "copy-starts-at-C":
        event(b, C)
    elif kind == "copy-spans-C":
        event(b, C - 6)
    elif kind == "zeros-span-C":
        b.fill(C - 20 - b.pos())
        z = b.raw(bytes(40))
        b.accept("zeros", z + 1, z, z, z + 40, must=True)
    elif kind == "run-spans-C":
        b.fill(C - 23 - b.pos())
        u = b.fill(3)
        x = b.copy(u, 40)
        b.accept("runlen", x, u, x, x + 40, must=True)
    elif kind == "copy-ends-at-C+O-1":
        event(b, C + O - 1 - 12)
    elif kind == "copy-ends-at-C+O+1":
        event(b, C + O + 1 - 12)
    elif kind == "copy-starts-at-C+O-1":
        event(b, C + O - 1)
    elif kind == "copy-starts-at-C+O+15":
        event(b, C + O + 15)
    elif src is not None:
        b.fill(C + 100 - b.pos())
        x = b.copy(src, 12)
        b.accept("window", x, src, x, x + 12, must=True)
        event(b, C + 500)
    else:
        assert kind == "no-copy-end-in-overlap"
    b.fill(C + O + 300 - b.pos())
    for k in (2, 3):  # every later chunk start has a copy end 312 bytes past it
        if k * C + O + 400 < n:
            sparse(b, k * C - 100)
            event(b, k * C + 300, must=False)
    sparse(b, n)
    assert n < 3 * C or n > 3 * C + O + 400


K1C_KINDS = (
    ("copy-ends-at-C", 72), ("copy-starts-at-C", 80), ("copy-spans-C", 100), ("zeros-span-C", 72), ("run-spans-C", 76),
    ("source-beyond-warmup", 84), ("source-within-warmup", 72), ("no-copy-end-in-overlap", 92),
    ("copy-ends-at-C+O-1", 72), ("copy-ends-at-C+O+1", 88), ("copy-starts-at-C+O-1", 72), ("copy-starts-at-C+O+15", 76),
)


def group_i():
    """(the two cases whose source lies thousands of positions back use a 4,096-entry table, the
    largest K1c takes: in a 1,024-entry one no entry lasts that long)"""
    return [
        make(f"I-{kind}", lambda b, kind=kind, k=k: k1c_stream(b, kind, k * KiB + 5 * k), 10000 + j, htable=4096 if kind.startswith("source") else 1024)
        for j, (kind, k) in enumerate(K1C_KINDS)
    ]


def k1x_stream(b: Build, at, n: int):
    """n bytes of filler with one 10-byte copy from 60 back at each position of `at`."""
    b.events = None
    for x in at:
        event(b, x, 10, 60)
    b.fill(n - b.pos())


def k1x_from(b: Build, n: int):
    """A copy of 6 bytes whose source starts exactly where the copy before it ends -- where K1x's
    next round starts (`from`).  The entries of the source's second and third four-gram are
    overwritten, so only a candidate at `from` itself finds it."""
    b.events = None
    event(b, 9000, 10, 60)
    s = b.fill(6)
    b.fill(3)
    for k in (1, 2):
        b.raw(b.collider(bytes(b.d[s + k : s + k + 4])))
        b.fill(1)
    b.fill(40)
    y = b.copy(s, 6)
    b.accept("runlen", y, s, y, y + 6, must=True)
    event(b, 30000, 10, 60)
    b.fill(n - b.pos())


def keep_bucket_free(b: Build, s: int, x: int):
    """Redraw filler bytes until no position in (s, x) has the hash of the four-gram at s: the
    entry made at s (and kx_pred's chain of that hash) then reaches x untouched.  The bytes of
    the source [s, s + 10) and the byte x - 1 next to the plant keep their rules."""
    d = np.frombuffer(bytes(b.d[:x]) + bytes(b.d[s : s + 3]), np.uint8).astype(np.uint32)
    h = gram_hash(bytes(b.d[s : s + 4]), b.htable)
    sh = np.uint32(32 - (b.htable - 1).bit_length())
    for _ in range(200):
        u = d[:-3] | d[1:-2] << 8 | d[2:-1] << 16 | d[3:] << 24
        bad = np.nonzero(((u * np.uint32(0x1E35A7BD)) >> sh)[s + 1 : x] == h)[0] + s + 1
        if not len(bad):
            break
        for p in bad:
            q = min(int(p) + 3, x - 1)
            if q < s + 10:
                raise Retry
            d[q] = b.rng.integers(1, 256)
    else:
        raise Retry
    b.d[:x] = d[:x].astype(np.uint8).tobytes()


def k1x_pred(b: Build, off: int, n: int):
    """kx_pred's u16 distance at its edge.  The plant's first four-gram is the last position
    of K1x's chunk 1 (32,767), its source at chunk offset `off`, and no position between has
    the source's hash: off = 0 is the largest chunk-local distance, 16,383; off = 1 the next;
    off = -1 puts the source in chunk 0, 16,384 back, so the chunk's incoming entry finds it."""
    b.events = None
    x = 2 * KX_C - 1
    s = KX_C + off
    b.fill(x)
    keep_bucket_free(b, s, x)
    at = b.copy(s, 10)
    b.accept("runlen", at, s, at, at + 10, must=True)
    event(b, 36000, 10, 60)
    b.fill(n - b.pos())


def group_j():
    cases = []
    for off in (0, 1, -1):
        cases.append(make(f"J-predecessor-{KX_C - 1 - off}-back", lambda b, off=off: k1x_pred(b, off, 41 * KiB), 11300 + off))
    for j, (E, k) in enumerate(((0, 40), (1, 44), (7, 48), (8, 52), (9, 64), (20, 80))):
        n = k * KiB + 3 * E + 1
        at = [(e + 1) * (n // (E + 1)) - 7 * e for e in range(E)]
        cases.append(make(f"J-{E}-events", lambda b, at=at, n=n: k1x_stream(b, at, n), 11000 + j))
    for x in (KX_C - 1, KX_C, KX_C + 1):
        cases.append(make(f"J-event-at-{x}", lambda b, x=x: k1x_stream(b, [5000, x, 30000], 41 * KiB), 11100 + x % 8))
    cases.append(make("J-source-at-previous-copy-end", lambda b: k1x_from(b, 42 * KiB), 11150))
    for gap in (100, 255, 256, 257):
        at = [9000, 9000 + gap, 9000 + 2 * gap, 9000 + 3 * gap, 30000]
        cases.append(make(f"J-events-{gap}-apart", lambda b, at=at: k1x_stream(b, at, 43 * KiB), 11200 + gap % 8))
    return cases


# ------------------------------------------------------------------ the groups, built once


@functools.lru_cache(maxsize=None)
def group(name: str):
    return tuple(
        {
            "A": group_a, "B": group_b, "C": group_c, "D": group_d, "E": group_e, "F": group_f, "G": group_g,
            "Glong": group_g_long, "H1024": lambda: group_h(1024), "H4096": lambda: group_h(4096),
            "I": group_i, "J": group_j,
        }[name]()
    )


GROUPS = ("A", "B", "C", "D", "E", "F", "G", "Glong", "H1024", "H4096", "I", "J")
