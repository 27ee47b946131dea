"""Write sequences for a Writer handle whose parse by Go is known before the oracle runs.

TEST INFRASTRUCTURE ONLY.  tests/k1_inputs.py builds single-Write fresh streams; none of them
reaches the handle's own code: K1L parsing against history in a ring (RingSrc / LdsSrc), a table
that survives from one launch to the next, the kernels that store a Write into the ring.  A case
here is a handle configuration (block, htable, positions set through the testing hook), a list of
Writes -- history first, the Write under test last -- and what Go must make of the Write under
test: its token list (`tokens`), or the tokens that carry the edge (`named`), and pyoracle's trace
events (positions relative to the Write under test: a candidate in the ring is negative).

The bytes are laid down with k1_inputs.Build (filler in 1..255, forced-different neighbours of a
planted repeat, colliders) over the concatenation of the Writes; cut() ends a Write.  A builder is
tried with up to SEEDS seeds until the C oracle's tokens and pyoracle's trace are the intended
ones, and raises Unbuildable when it runs out.

The table holds the last few thousand scanned positions only, so a source far back is reachable
only when nothing scanned since has taken its bucket.  Far histories are therefore a random unit
followed by repetitions of it: Go jumps over the repetitions in one copy and inserts two positions,
and the first unit's entries stand (R3).  R4's echo needs a live entry every few bytes of a whole
window and lays its own (echo())."""

from __future__ import annotations

import functools

import numpy as np

import k1_inputs as ki
import oracle as orc
import pyoracle as po
from k1_inputs import Retry, Unbuildable, tokens_of

KiB = 1 << 10
SEEDS = ki.SEEDS
LDS_WRITE = 49152  # a Write up to this long is staged in LDS by K1L (kHandleLdsWrite)
P32 = 1 << 32


def lit(n):
    return ("l", n)


def cpy(n, d):
    return ("c", n, d)


# ------------------------------------------------------------------ the oracles, Write by Write


def oracle_writes(block, htable, writes, pos=None):
    """The C oracle's bytes for each Write of the sequence (pos: {Write index: position set before it})."""
    w = orc.Writer(block, htable)
    outs = []
    for j, p in enumerate(writes):
        if pos and j in pos:
            w.set_pos(pos[j])
        n, e = w.write(p)
        assert e == 0 and n == len(p), (j, n, e)
        outs.append(w.sink)
        w.sink_clear()
    return outs


def py_writes(block, htable, writes, pos=None, under=None):
    """pyoracle's bytes per Write and its trace of the Write under test."""
    w = po.Writer(block, htable)
    outs, trace = [], []
    for j, p in enumerate(writes):
        if pos and j in pos:
            w.pos = pos[j]
        w.trace = trace if j == under else None
        at = len(w.sink)
        n, e = w.write(p)
        assert e == 0 and n == len(p), (j, n, e)
        outs.append(w.sink[at:])
    return outs, trace


# ------------------------------------------------------------------ the builder


class Seq(ki.Build):
    """k1_inputs.Build over the concatenated Writes.  Positions are offsets in the concatenation."""

    def __init__(self, seed, htable=1024):
        super().__init__(seed, htable)
        self.bounds = []  # the Writes' ends
        self.want = None  # the Write under test's whole token list, or None
        self.named = []  # tokens it must hold, in this order
        self.wpos = {}  # {Write index: stream position set before it}
        self.calls = None  # the Writes of each call, where the case fixes them (R6)
        self.unread = None  # echo cases: the kept bytes the echo's copies need not read (the first ones)

    def cut(self) -> int:
        """End the Write; -> where the next one starts."""
        self.bounds.append(len(self.d))
        self.avoid = None
        return len(self.d)

    def writes(self):
        at = [0] + self.bounds
        assert self.bounds and self.bounds[-1] == len(self.d)
        return [bytes(self.d[a:b]) for a, b in zip(at, at[1:])]

    def bulk(self, k: int) -> None:
        """k bytes of cheap history: filler, or past 2,000 bytes a unit of 400 and its repetitions."""
        if k <= 2000:
            self.fill(k)
        else:
            u = self.fill(400)
            self.copy(u, k - 400)
            self.avoid = None


class WCase:
    def __init__(self, name, b: Seq, block, htable, seed, comps, py):
        self.name, self.block, self.htable, self.seed = name, block, htable, seed
        self.writes, self.pos, self.calls = b.writes(), dict(b.wpos), b.calls
        self.under = len(self.writes) - 1
        self.tokens, self.named = b.want, list(b.named)
        self.must, self.far, self.short, self.unread = list(b.must), list(b.far), list(b.short), b.unread
        self.comps, self._py = comps, py

    def py(self):
        """(pyoracle's bytes per Write, its trace of the Write under test); run on first use where
        the seed search did not need the trace (pyoracle counts an echo's long matches byte by byte)."""
        if self._py is None:
            self._py = py_writes(self.block, self.htable, self.writes, self.pos, self.under)
        return self._py

    py_comps = property(lambda self: self.py()[0])
    trace = property(lambda self: self.py()[1])

    def starts(self):
        """The stream position of every Write's first byte."""
        at, out = 0, []
        for j, p in enumerate(self.writes):
            at = self.pos.get(j, at)
            out.append(at)
            at += len(p)
        return out

    def __repr__(self):
        return f"WCase({self.name}, Writes of {[len(p) for p in self.writes]}, seed {self.seed})"


def holds_in_order(toks, named) -> bool:
    it = iter(toks)
    return all(any(t == want for t in it) for want in named)


def verdict(b: Seq, block, htable):
    ws = b.writes()
    under = len(ws) - 1
    comps = oracle_writes(block, htable, ws, b.wpos)
    got = tokens_of(comps[under])[0]
    if b.want is not None and got != b.want:
        return None, f"tokens {got[:10]} ..., intended {b.want[:10]} ..."
    if not holds_in_order(got, b.named):
        return None, f"tokens {got[:10]} ... lack {b.named}"
    if not (b.must or b.far or b.short):
        return (comps, None), None
    py_comps, trace = py_writes(block, htable, ws, b.wpos, under)
    assert py_comps == comps, "pyoracle and the C oracle differ"
    acc = {e for e in trace if e[0] not in ("far", "short")}
    if not set(b.must) <= acc:
        return None, f"trace lacks {[e for e in b.must if e not in acc]}"
    if not set(b.far) <= {e[1] for e in trace if e[0] == "far"}:
        return None, f"far skips lack {b.far}"
    if not set(b.short) <= {e[1:] for e in trace if e[0] == "short"}:
        return None, f"refused candidates lack {b.short}"
    return (comps, (py_comps, trace)), None


def make(name, fn, seed, block, htable=1024) -> WCase:
    why = "every seed refused by the builder"
    for s in range(seed * SEEDS, (seed + 1) * SEEDS):
        b = Seq(s, htable)
        try:
            fn(b)
        except Retry:
            continue
        got, why = verdict(b, block, htable)
        if got is not None:
            return WCase(name, b, block, htable, s, *got)
    raise Unbuildable(f"{name}: no seed of {SEEDS} gives the intended parse; the last: {why}")


# ------------------------------------------------------------------ R1: the Write's start

R1_K = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24)
R1_LURE_Y = (0, 1, 2, 7, 8, 9)
R1_CAND_Y = (-24, -17, -16, -15, -9, -8, -7, 0, 1, 7, 8, 9)
R1_BS = 65536


def split(b: Seq, k: int):
    """A 40-byte repeat whose source begins k bytes before the Write, found while nothing is emitted
    yet (done = 0).  Go's forward count stops at the stream position of done: the ring does not hold
    the Write yet.  k >= 6: two copies at one distance, k bytes from the ring and 40 - k found again at
    the Write's first byte; k < 6 (k < 4: the ring part's four-gram straddles the two Writes and was
    never inserted): the ring part is refused and the rest found from the Write's first byte."""
    b.fill(50)
    h = b.cut()
    b.fill(40 - k)
    b.fill(9)
    x = b.copy(h - k, 40) - h
    b.fill(20)
    b.cut()
    if k >= 6:
        b.want = [lit(x), cpy(k, x + k), cpy(40 - k, x + k), lit(20)]
        b.must += [("window", x, -k, x, x + k), ("window", x + k, 0, x + k, x + 40)]
    else:
        b.want = [lit(x + k), cpy(40 - k, x + k), lit(20)]
        b.must.append(("runlen", x + k, 0, x + k, x + 40))
        if k >= 4:
            b.short.append((x, -k))


def lure(b: Seq, y: int):
    """The Write's bytes 0 .. y+12 again with the ring's last 12 bytes in front of them, accepted at the
    candidate y (the entries of positions 0 .. y-1, and of the ring's last 12 bytes, are overwritten by
    colliders) and found backward to the Write's first byte, not into the ring."""
    b.fill(50)
    h = b.cut()
    b.fill(y + 12)
    b.fill(8)
    for j in list(range(-12, -3)) + list(range(y)):
        b.raw(b.collider(bytes(b.d[h + j : h + j + 4])))
        b.fill(1)
    b.fill(3)
    x = b.raw(bytes(b.d[h - 12 : h + y + 12])) - h
    b.avoid = b.d[h + y + 12]
    b.fill(15)
    b.cut()
    b.want = [lit(x + 12), cpy(y + 12, x + 12), lit(15)]
    b.must.append(("runlen", x + 12 + y, y, x + 12, x + 24 + y))


def cand_at(b: Seq, y: int):
    """A 10-byte source at position y of the Write (y < 0: in the ring, the last bytes of the Write
    before; -9 .. -7: it runs into the Write and Go keeps the ring part) found at its first byte.
    y = 0: the byte before the plant is the ring's last, and nothing is found backward."""
    b.fill(50)
    h = b.cut()
    if y < 0:
        b.fill(max(0, y + 10))
        b.fill(7)
        x = b.copy(h + y, 10) - h
        b.fill(15)
        k = min(-y, 10)
        b.want = [lit(x), cpy(k, x - y), lit(10 - k + 15)]
        b.must.append(("window", x, y, x, x + k))
    else:
        b.fill(y)
        b.fill(10)
        b.fill(7)
        if y == 0:
            b.d[-1] = b.d[h - 1]
            x = b.raw(bytes(b.d[h : h + 10])) - h
            b.avoid = b.d[h + 10]
        else:
            x = b.copy(h + y, 10) - h
        b.fill(15)
        b.want = [lit(x), cpy(10, x - y), lit(15)]
        b.must.append(("runlen", x, y, x, x + 10))
    b.cut()


def group_r1():
    cases = [make(f"R1-source-{k}-before", lambda b, k=k: split(b, k), 100 + k, R1_BS) for k in R1_K]
    cases += [make(f"R1-lure-at-{y}", lambda b, y=y: lure(b, y), 140 + y, R1_BS) for y in R1_LURE_Y]
    cases += [make(f"R1-candidate-at-{y}", lambda b, y=y: cand_at(b, y), 180 + y, R1_BS) for y in R1_CAND_Y]
    return cases


# ------------------------------------------------------------------ R2: the ring's end

R2_RES = (0, 1, 7, 8, 9, 15)
R2_SPLIT = (1, 7, 8, 9, 15, 16, 17, 31)


def wrap(b: Seq, bs: int, res: int, long_prefix: bool, sp: int):
    """A prefix Write of res bytes (the general kernel; res = 0: an empty Write) or 16 + res (K1L),
    a history Write that ends at a position of residue res mod 16, and in it a 48-byte source with
    sp bytes in the ring's last slots and 48 - sp in its first ones; the Write under test is 5 bytes,
    the 48 again, 12 bytes."""
    pre = res + (16 if long_prefix else 0)
    b.fill(pre)
    b.cut()
    s = bs - sp
    start = s + 48 + 4
    start += (res - start) % 16
    b.bulk(s - 80 - pre)
    b.fill(80)
    assert b.pos() == s
    b.fill(48)
    b.fill(start - s - 48)
    b.cut()
    b.fill(5)
    x = b.copy(s, 48)
    b.fill(12)
    b.cut()
    b.want = [lit(5), cpy(48, x - s), lit(12)]
    b.must.append(("window", 5, s - start, 5, 53))


def group_r2():
    cases = []
    combos = [(res, lp) for res in R2_RES for lp in (False, True)]
    for res, lp in combos:
        for sp in R2_SPLIT:
            cases.append(make(f"R2-bs1024-start{res}{'+16' if lp else ''}-wrap-after-{sp}", lambda b, res=res, lp=lp, sp=sp: wrap(b, 1024, res, lp, sp), 300 + res + sp, 1024))
    for res, lp in combos:
        for sp in R2_SPLIT:
            cases.append(make(f"R2-bs65536-start{res}{'+16' if lp else ''}-wrap-after-{sp}", lambda b, res=res, lp=lp, sp=sp: wrap(b, 65536, res, lp, sp), 400 + res + sp, 65536))
    return cases


# ------------------------------------------------------------------ R3: the staged extent

R3_D = (-24, -9, -8, -7, -1, 0, 1, 7, 8, 9, 24)
R3_RL = 32768  # kLdsRing: K1L stages min(bs, 32,768) ring bytes before the Write


def staged(b: Seq, bs: int, d: int, L: int, P: int = 5):
    """The candidate of an L-byte plant at y = -rl + d, rl = min(bs, 32,768), with P bytes pending.  The
    history is filler, a unit that holds the source, and the unit's repetitions up to rl + 64 bytes.
    bs > rl: a copy of L bytes.  bs = rl: y = -bs + d, and the candidate is far for d < 0 (and every
    later one of the plant until -bs itself), else Go trims the copy to the d - P bytes that the ring
    still holds when the copy's last byte is written: no copy below 6."""
    rl = min(bs, R3_RL)
    a, n = 10, rl + 64
    pre = n - rl + d - a
    b.fill(pre)
    u = b.fill(a + L + 30)
    b.copy(u, n - b.pos())
    start = b.cut()
    assert u + a - start == -rl + d
    b.fill(P)
    b.copy(u + a, L)
    b.fill(15)
    b.cut()
    if bs > rl:
        b.want = [lit(P), cpy(L, P + rl - d), lit(15)]
        b.must.append(("window", P, -rl + d, P, P + L))
    elif d - P >= 6:
        b.named = [cpy(d - P, P + bs - d)]
        b.must.append(("window", P, -bs + d, P, d))
    else:
        b.want = [lit(P + L + 15)]
        if d < 0:
            b.far.append(P)
        else:
            b.short.append((P, -bs + d))


def group_r3():
    cases = []
    for L in (40, 200):
        cases += [make(f"R3-bs65536-at-rl{d:+d}-len{L}", lambda b, d=d, L=L: staged(b, 65536, d, L), 500 + d + L, 65536) for d in R3_D]
    for bs in (32768, 16384):
        cases += [make(f"R3-bs{bs}-at-bs{d:+d}", lambda b, d=d, bs=bs: staged(b, bs, d, 40), 600 + d + bs % 7, bs) for d in R3_D]
        cases += [make(f"R3-bs{bs}-{bs - d}-back", lambda b, d=d, bs=bs: staged(b, bs, d, 40, 0), 650 + d + bs % 7, bs) for d in (1, 0, -1)]
    return cases


# ------------------------------------------------------------------ R4: lengths and the ring store

R4_LEN = (0, 1, 5, 15, 16, 17, 49151, 49152, 49153)
R4_BS = (1024, 4096, 16384, 65536)
R4_RES = (0, 9)


def length(b: Seq, n: int):
    """A Write of exactly n bytes after 64 bytes of history: its planted repeat first, filler after."""
    b.fill(64)
    h = b.cut()
    if n < 15:
        b.fill(n)
        b.want = [lit(n)] if n else []
    else:
        pl = 8 if n < 20 else 12
        b.fill(3)
        b.copy(20, pl)
        b.fill(n - 3 - pl)
        b.want = [lit(3), cpy(pl, h + 3 - 20), lit(n - 3 - pl)]
    b.cut()


def echo_lengths(bs: int):
    return sorted({bs - 1, bs, bs + 1, 2 * bs + 5, 16, 17, 49151, 49152, 49153})


ECHO_CAP = 16  # the first kept bytes an echo may leave unread
ECHO_COPIES = 970  # the most copies, each with a live table entry of its own, an echo is built with
ECHO_DUMP = 32  # buckets set aside for the second position of every copy


def echo_plan(bs: int, L: int):
    """(u, step) of echo(): the echo starts u bytes into the kept bytes and its copies are step =
    bs - kept + u bytes long.  u <= ECHO_CAP wherever that takes at most ECHO_COPIES copies whose last
    one is whole or at least a copy (6 bytes): u = 0 if a copy may be 16 bytes without it, else the
    largest such u (the fewest copies).  Else (echo_cap_reachable) step is doubled from 32 until
    ECHO_COPIES suffice."""
    kept = min(L, bs)
    slack = bs - kept
    for u in range(ECHO_CAP + 1) if slack >= ECHO_CAP else range(ECHO_CAP, -1, -1):
        step = slack + u
        if step >= 16 and -(-(kept - u) // step) <= ECHO_COPIES and (kept - u) % step in (0, *range(6, step)):
            return u, step
    step = 32
    while -(-kept // step) > ECHO_COPIES:
        step *= 2
    return step - slack, step


def echo_cap_reachable(bs: int, L: int) -> bool:
    """Whether an echo is built to read every kept byte but the first ECHO_CAP.  Each of its copies
    is at most bs - kept + 16 bytes and is found only through a table entry at its own first position:
    a bucket of its own, which nothing either Write inserts later may take before the echo looks it
    up -- and both insert a position whenever they look one up.  A full ring (or one byte short) of
    65,536 takes 3,855 copies, more than the table has buckets: impossible.  A full ring of 16,384
    takes 1,023: with one bucket for the second position that the echo inserts after every copy that
    is all 1,024, every other four-gram of every head with a prescribed bucket: out of a search's
    reach.  963 copies (16,383 bytes kept of 16,384) are built."""
    kept = min(L, bs)
    return -(-(kept - ECHO_CAP) // (bs - kept + ECHO_CAP)) <= ECHO_COPIES


def _buckets(g, htable):
    return (g * np.uint32(0x1E35A7BD)) >> np.uint32(32 - (htable - 1).bit_length())


def pick_head(b: Seq, tail: bytes, ok0, ok1, ok23, prev, ban0):
    """Four fresh bytes in front of `tail` whose four four-grams fall into allowed buckets: the first
    (the copy's own entry) where ok0, the second where ok1, the others where ok23, and none of the
    later three into the first one's.  Its first byte is none of ban0 and its last differs from prev's."""
    t = [np.uint32(v) for v in tail[:3]]
    for k in range(600):
        c = b.rng.integers(1, 256, (8192 if k > 1 else 256, 4), dtype=np.uint32)
        g = [
            c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16 | c[:, 3] << 24,
            c[:, 1] | c[:, 2] << 8 | c[:, 3] << 16 | t[0] << 24,
            c[:, 2] | c[:, 3] << 8 | t[0] << 16 | t[1] << 24,
            c[:, 3] | t[0] << 8 | t[1] << 16 | t[2] << 24,
        ]
        h = [_buckets(x, b.htable) for x in g]
        good = ok0[h[0]] & ok1[h[1]] & ok23[h[2]] & ok23[h[3]] & (h[0] != h[1]) & (h[0] != h[2]) & (h[0] != h[3])
        if prev is not None:
            good &= (c[:, 3] != prev[3]) & ~np.isin(c[:, 0], list(ban0))
        if b.avoid is not None:
            good &= c[:, 0] != b.avoid
        k = np.nonzero(good)[0]
        if len(k):
            return bytes(int(v) for v in c[k[0]]), int(h[0][k[0]])
    raise Retry


def echo(b: Seq, bs: int, L: int, res: int):
    """A Write A of L bytes at position res, and an echo Write whose copies read what the ring keeps
    of A (its last kept = min(L, bs) bytes).

    Go trims a copy to the bytes the ring still holds when the copy's LAST byte is written: a copy of
    n bytes at distance D needs n <= bs - D.  An echo that starts u bytes into the kept bytes has
    D = kept - u, so its copies are at most step = bs - kept + u bytes long, and each needs a live
    table entry where it starts.  A of up to 64 bytes is filler and the echo is A itself: one copy,
    u = 0.  Longer ones are u bytes of filler and chunks of step bytes (echo_plan) -- four fresh bytes
    (the head) and a shared tail that Go copies from the chunk before, so that a chunk inserts its
    head's four positions and positions of the tail whose buckets the first chunk's tail took already.
    The heads are chosen (pick_head) so that a head's first four-gram has a bucket that nothing else
    in either Write is inserted into: not the tail's, not another head's, and the heads' second
    four-grams (which the echo inserts too, after each copy) go to ECHO_DUMP buckets set aside.  Every
    copy of the echo then ends where a chunk does and the next finds its head.  A tail over 600 bytes
    is a unit of 200 and its repetitions, which Go does not insert.  What comes before the kept bytes
    (L > bs) is a unit and its repetitions."""
    if res:
        b.fill(res)
        b.cut()
    a0 = b.pos()
    kept = min(L, bs)
    if L <= 64:
        b.fill(L)
        b.cut()
        b.raw(bytes(b.d[a0 : a0 + L]))
        b.cut()
        b.want, b.unread = [cpy(L, L)], 0
        return
    u, step = echo_plan(bs, L)
    if L > kept:
        b.bulk(L - kept)
    k0 = b.pos()
    b.fill(u)
    if step - 4 > 600:
        unit = bytes(b.rng.integers(1, 256, 200, dtype=np.uint8))
        tail = (unit * (step // 200 + 1))[: step - 4]
        scanned = tail[:212]
    else:
        tail = scanned = bytes(b.rng.integers(1, 256, step - 4, dtype=np.uint8))
    tb = np.zeros(b.htable, bool)  # the buckets the tail's scanned positions take
    tb[[ki.gram_hash(scanned[t : t + 4], b.htable) for t in range(len(scanned) - 3)]] = True
    dump = np.zeros(b.htable, bool)
    dump[b.rng.choice(np.nonzero(~tb)[0], ECHO_DUMP, replace=False)] = True
    heads = np.zeros(b.htable, bool)
    prev, after = None, {}  # after[v]: the first bytes of the heads that follow a head ending in v
    while b.pos() < k0 + kept:
        # a head's last byte and the tail may be found at any earlier head that ends alike: that copy
        # must end with the tail too, or the next head's positions are never inserted
        ban0 = after.setdefault(prev[3], {prev[0]}) if prev else ()
        h, bucket = pick_head(b, tail, ~heads & ~tb & ~dump, dump, ~heads & ~tb, prev, ban0)
        if prev:
            ban0.add(h[0])
        heads[bucket] = True
        prev = h
        b.avoid = None
        b.d += (h + tail)[: k0 + kept - b.pos()]
    assert b.pos() == k0 + kept == a0 + L
    b.cut()
    b.raw(bytes(b.d[k0 + u : k0 + kept]))
    b.cut()
    n, b.want = kept - u, []
    assert step <= kept - u
    for at in range(0, n, step):
        b.want.append(cpy(min(step, n - at), kept - u))
    b.unread = u


def group_r4():
    cases = [make(f"R4-length-{n}", lambda b, n=n: length(b, n), 700 + n % 50, 65536) for n in R4_LEN]
    for bs in R4_BS:
        for L in echo_lengths(bs):
            for res in R4_RES:
                cases.append(make(f"R4-bs{bs}-echo-of-{L}-at-{res}", lambda b, bs=bs, L=L, res=res: echo(b, bs, L, res), 800 + L % 50 + res, bs))
    return cases


def ring_reads(c: WCase):
    """The stream positions before the Write under test that its copies read, as a sorted list of
    [from, to) ranges, read from the oracle's tokens."""
    start = c.starts()[c.under]
    at, got = start, []
    for t in tokens_of(c.comps[c.under])[0]:
        if t[0] == "c" and t[2]:
            lo, hi = at - t[2], min(at - t[2] + t[1], start)
            if lo < hi:
                got.append((lo, hi))
        at += t[1]
    return sorted(got)


# ------------------------------------------------------------------ R5: positions and the clamp


def at_position(b: Seq, end_at: int):
    """64 bytes of history and a 37-byte Write with a 12-byte repeat of it, the Write ending at end_at."""
    b.fill(64)
    h = b.cut()
    b.wpos[0] = end_at - 37 - 64
    b.fill(5)
    b.copy(30, 12)
    b.fill(20)
    b.cut()
    b.want = [lit(5), cpy(12, h + 5 - 30), lit(20)]


def starts_at_2_32(b: Seq):
    """A K1L Write that ends at 2^32 and the Write after it, which repeats 12 of its bytes."""
    b.fill(64)
    h = b.cut()
    b.wpos[0] = P32 - 64
    b.fill(5)
    b.copy(30, 12)
    b.fill(20)
    b.cut()
    b.want = [lit(5), cpy(12, h + 5 - 30), lit(20)]


def jump(b: Seq, back: bool):
    """64 bytes at position 0, then the position moves on by 2^28 + 100 with ring and table kept: every
    entry is far for the next Write (K1L clamps them all and leaves them alone in the handle's table),
    which repeats 12 of the first Write's bytes and must not find them.  back: the position is then set
    to 64 again, where the entries that the second Write did not overwrite are near once more, and a
    third Write finds its repeat of the first one's bytes in the ring."""
    b.fill(64)
    b.cut()
    far_at = 64 + (1 << 28) + 100
    b.wpos[1] = far_at
    b.fill(5)
    b.raw(bytes(b.d[30:42]))
    b.fill(20)
    b.cut()
    if not back:
        b.want = [lit(37)]
        b.far.append(5)
        return
    b.wpos[2] = 64
    b.fill(5)
    b.copy(10, 12)
    b.fill(20)
    b.cut()
    b.want = [lit(5), cpy(12, 64 + 5 - 10), lit(20)]
    b.must.append(("window", 5, 10 - 64, 5, 17))


def group_r5():
    return [
        make("R5-ends-at-2^32", lambda b: at_position(b, P32), 900, 65536),
        make("R5-ends-at-2^32+1", lambda b: at_position(b, P32 + 1), 901, 65536),
        make("R5-starts-at-2^32", starts_at_2_32, 902, 65536),
        make("R5-jump-2^28+100", lambda b: jump(b, False), 903, 65536),
        make("R5-jump-and-back", lambda b: jump(b, True), 904, 65536),
    ]


# ------------------------------------------------------------------ R6: several Writes in one call


def chain(b: Seq, lens, calls, echo_len: int = 0):
    """Writes of the given lengths; each of 30 bytes or more after the first starts with 7 bytes and
    12 bytes from the end of the last such Write before it.  echo_len: a last Write that repeats that
    many bytes which end 20 bytes before it."""
    src = None
    for n in lens:
        at = b.pos()
        if n >= 30 and src is not None:
            b.fill(7)
            b.copy(src, 12)
            b.fill(n - 19)
            b.want = [lit(7), cpy(12, at + 7 - src), lit(n - 19)]
        else:
            b.fill(n)
        if n >= 30:
            src = b.pos() - 20
        b.cut()
    if echo_len:
        at = b.pos()
        b.fill(7)
        b.copy(at - 20 - echo_len, echo_len)
        b.fill(9)
        b.cut()
        b.want = [lit(7), cpy(echo_len, 7 + 20 + echo_len), lit(9)]
    b.calls = calls


R6 = (
    ("k2-zero-copy", 65536, (40, 60), [[0, 1]], 0),
    ("k3-zero-copy", 65536, (40, 60, 100), [[0, 1, 2]], 0),
    ("k4-zero-copy", 65536, (40, 16, 49152, 3000), [[0, 1, 2, 3]], 0),
    ("k2-staged", 65536, (49153, 60), [[0, 1]], 0),
    ("k3-staged", 65536, (40, 49153, 100), [[0, 1, 2]], 0),
    ("k4-staged", 65536, (40, 60, 100, 49153), [[0, 1, 2, 3]], 0),
    ("k3-with-empty-Write", 65536, (40, 0, 60), [[0, 1, 2]], 0),
    ("k3-with-5-byte-Write", 65536, (40, 5, 60), [[0, 1, 2]], 0),
    ("bs1024-call-longer-than-window-multi", 1024, (500, 5, 600), [[0, 1, 2], [3]], 40),
    ("bs1024-call-longer-than-window-k1l", 1024, (500, 600), [[0, 1], [2]], 40),
)


def group_r6():
    return [make(f"R6-{name}", lambda b, lens=lens, calls=calls, e=e: chain(b, lens, calls, e), 950 + j, bs) for j, (name, bs, lens, calls, e) in enumerate(R6)]


# ------------------------------------------------------------------ the groups, built once


@functools.lru_cache(maxsize=None)
def group(name: str):
    return tuple({"R1": group_r1, "R2": group_r2, "R3": group_r3, "R4": group_r4, "R5": group_r5, "R6": group_r6}[name]())


GROUPS = ("R1", "R2", "R3", "R4", "R5", "R6")
