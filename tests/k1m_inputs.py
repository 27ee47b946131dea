"""Write sequences for fresh multi-Write streams whose parse by Go is known before the oracle runs.

TEST INFRASTRUCTURE ONLY.  tests/k1_inputs.py builds single-Write streams and tests/k1w_inputs.py
Write sequences for a handle (a ring, a table that lives from one launch to the next).  Neither
reaches the code that ez_compress_batch_writes alone runs: k1_parse<G, T16, MW = true>, whose windows,
caps and guards follow the current Write's first and last byte (wstart, wend), and the general
kernel's multi-Write variant without a ring, which re-bases its view of the input at every Write.
A case here is a fresh stream (block, htable), its Writes, and what Go must make of some of them:
`want_at[j]`, the whole token list of Write j (stated for the Write under test and for every Write
after it), and per stated Write pyoracle's trace events -- accepted matches (`must_at`), candidates
looked at and refused (`short_at`), free-form checks (`check_at`).  Positions in a trace are relative
to that Write's first byte: a candidate in an earlier Write is negative and Go takes it in the
window branch (the block holds it), one in the Write itself in the run-length branch.

The bytes are laid with k1w_inputs.Seq (k1_inputs.Build over the concatenated Writes: filler in
1..255, forced-different neighbours of a planted repeat, colliders; cut() ends a Write).  make() and
verdict() are k1w_inputs' with the one Write under test replaced by any number of stated Writes: a
builder is tried with up to SEEDS seeds until the C oracle's tokens and pyoracle's trace are the
intended ones, and make() raises Unbuildable when it runs out.

Unless a group says otherwise: block 65,536, table 1,024, streams under 400 bytes."""

from __future__ import annotations

import functools

import k1_inputs as ki
import k1w_inputs as kw
import pyoracle as po
from k1_inputs import Retry, Unbuildable, tokens_of
from k1w_inputs import Seq, cpy, lit

MiB = 1 << 20
SEEDS = ki.SEEDS
BLOCK, HTABLE = 65536, 1024


# ------------------------------------------------------------------ the builder and the oracles


class MSeq(Seq):
    """k1w_inputs.Seq with the intended parse kept per Write."""

    def __init__(self, seed, htable=HTABLE):
        super().__init__(seed, htable)
        self.want_at = {}  # {Write index: its whole token list}
        self.must_at = {}  # {Write index: accepted matches its trace must hold}
        self.short_at = {}  # {Write index: (i, candidate) it must look at in the block and refuse}
        self.check_at = {}  # {Write index: [(what, fn(trace) -> bool)]}
        self.c_only = False  # a long stream: the stated tokens are held by the C oracle alone

    def zeros(self, k: int) -> int:
        at = len(self.d)
        self.d += bytes(k)
        self.avoid = None
        return at


def py_traces(block, htable, writes):
    """pyoracle's bytes per Write and its trace of every Write."""
    w = po.Writer(block, htable)
    outs, traces = [], []
    for p in writes:
        w.trace = []
        at = len(w._sink)
        n, e = w.write(p)
        assert e == 0 and n == len(p)
        outs.append(bytes(w._sink[at:]))
        traces.append(w.trace)
    return outs, traces


def trace_lacks(b_or_case, traces):
    """The first stated trace event that the traces lack, as a sentence; None: they hold them all."""
    for j, must in b_or_case.must_at.items():
        acc = {e for e in traces[j] if e[0] not in ("far", "short")}
        if not set(must) <= acc:
            return f"Write {j}: trace lacks {[e for e in must if e not in acc]}, has {sorted(acc)[:6]}"
    for j, short in b_or_case.short_at.items():
        if not set(short) <= {e[1:] for e in traces[j] if e[0] == "short"}:
            return f"Write {j}: refused candidates lack {short}"
    for j, checks in b_or_case.check_at.items():
        for what, fn in checks:
            if not fn(traces[j]):
                return f"Write {j}: {what}"
    return None


def verdict(b: MSeq, block, htable):
    ws = b.writes()
    comps = kw.oracle_writes(block, htable, ws)
    for j, want in b.want_at.items():
        got = tokens_of(comps[j])[0]
        if got != want:
            return None, f"Write {j}: tokens {got[:8]} ..., intended {want[:8]} ..."
    if b.c_only:
        return (comps, None), None
    py_comps, traces = py_traces(block, htable, ws)
    assert py_comps == comps, "pyoracle and the C oracle differ"
    why = trace_lacks(b, traces)
    if why:
        return None, why
    return (comps, traces), None


class MCase:
    def __init__(self, name, b: MSeq, block, htable, seed, comps, traces):
        self.name, self.block, self.htable, self.seed = name, block, htable, seed
        self.writes = tuple(b.writes())
        self.want_at, self.must_at, self.short_at, self.check_at = dict(b.want_at), dict(b.must_at), dict(b.short_at), dict(b.check_at)
        self.under = min(b.want_at)  # the Write under test: every Write from it on is stated
        self.c_only = b.c_only
        self.comps, self.traces = comps, traces

    def starts(self):
        at, out = 0, []
        for p in self.writes:
            out.append(at)
            at += len(p)
        return out

    data = property(lambda self: b"".join(self.writes))

    def __repr__(self):
        return f"MCase({self.name}, Writes of {[len(p) for p in self.writes]}, seed {self.seed})"


def make(name, fn, seed, block=BLOCK, htable=HTABLE) -> MCase:
    why = "every seed refused by the builder"
    for s in range(seed * SEEDS, (seed + 1) * SEEDS):
        b = MSeq(s, htable)
        try:
            fn(b)
        except Retry:
            continue
        assert b.want_at and set(b.want_at) == set(range(min(b.want_at), len(b.bounds))), name
        got, why = verdict(b, block, htable)
        if got is not None:
            return MCase(name, b, block, htable, s, *got)
    raise Unbuildable(f"{name}: no seed of {SEEDS} gives the intended parse; the last: {why}")


# ------------------------------------------------------------------ M1: the Write's end, forward

M1_E = (1, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 40)
M1_E_SHORT = (6, 9, 15)  # with 8 more bytes instead of 40: the whole repeat is shorter than the capped count of 24


def ends_in_repeat(b: MSeq, e: int, same: bool, more: int = 40):
    """A source of e + more bytes, and a Write that ends with its first e bytes: Go's forward count
    stops at len(p).  e >= 6: one copy of exactly e ends the Write, no trailing literal; e < 6: no
    copy (e = 4, 5: the candidate is looked at and refused).  The next Write is the source's other
    `more` bytes and filler: found from its first byte with done at the Write's start, a second copy at
    the same distance.  same: the source lies in the Write under test (the run-length branch);
    else in the Write before (the window branch)."""
    b.fill(20)
    if not same:
        s = b.fill(e + more)
        b.fill(15)
    h = b.cut()
    b.fill(10 if same else 30)
    if same:
        s = b.fill(e + more)
        b.fill(15)
    x = b.copy(s, e)
    h2 = b.cut()
    b.raw(bytes(b.d[s + e : s + e + more]))
    b.avoid = b.d[s + e + more]
    b.fill(12)
    b.cut()
    if e >= 6:
        b.want_at[1] = [lit(x - h), cpy(e, x - s)]
        b.must_at[1] = [("runlen" if same else "window", x - h, s - h, x - h, x - h + e)]
    else:
        b.want_at[1] = [lit(x - h + e)]
        if e >= 4 and not same:
            b.short_at[1] = [(x - h, s - h)]
    b.want_at[2] = [cpy(more, x - s), lit(12)]
    b.must_at[2] = [("window", 0, s + e - h2, 0, more)]


def group_m1():
    cases = []
    for same in (False, True):
        for e in M1_E:
            br = "runlen" if same else "window"
            cases.append(make(f"M1-{br}-{e}-bytes-to-the-end", lambda b, e=e, same=same: ends_in_repeat(b, e, same), 1000 + 50 * same + e))
        for e in M1_E_SHORT:
            cases.append(make(f"M1-{br}-{e}-bytes-to-the-end-8-more", lambda b, e=e, same=same: ends_in_repeat(b, e, same, 8), 1100 + 50 * same + e))
    return cases


# ------------------------------------------------------------------ M2: the last positions of a Write

M2_J = (0, 1, 2, 3, 7)


def met_late(b: MSeq, j: int, same: bool, k: int = 6):
    """A repeat of k + 4 + j bytes that ends the Write, n bytes long, and is first met k bytes into it,
    at x = n - 4 - j: the table entries of the source's first k four-grams are overwritten by colliders
    (k1w_inputs.lure), so Go accepts at x with k bytes backward and 4 + j forward.  k = 7, j = -1: the
    repeat could be met only at n - 3, which Go never visits: the Write is one literal.  A Write of 10
    bytes follows.  same: source in the Write under test (run-length branch), else in the one before."""
    L = k + 4 + j
    b.fill(20)
    if not same:
        t = b.fill(L)
        b.fill(9)
    h = b.cut()
    b.fill(12)
    if same:
        t = b.fill(L)
        b.fill(9)
    for q in range(k):
        b.raw(b.collider(bytes(b.d[t + q : t + q + 4])))
        b.fill(1)
    b.fill(3)
    rep = b.copy(t, L)
    n = b.cut() - h
    b.fill(10)
    b.cut()
    if j >= 0:
        b.want_at[1] = [lit(rep - h), cpy(L, rep - t)]
        b.must_at[1] = [("runlen" if same else "window", rep + k - h, t + k - h, rep - h, n)]
    else:
        b.want_at[1] = [lit(n)]
    b.want_at[2] = [lit(10)]


M2_LANES = (7, 15, 31)


def extra_insert(b: MSeq, back: int, lane: int):
    """Writer.go:315-318 inserts xa + 1 after a window match accepted at xa when xa + 1 + 4 <= len(p).
    A 10-byte repeat of the Write before ends the Write under test (n bytes) and is accepted at
    xa = n - back (met_late with k = 10 - back): back = 5 inserts n - 4, the Write's last four bytes;
    back = 4 inserts nothing, the four-gram at n - 3 has one byte in the next Write.  A Write of 5 bytes
    follows, and then one that holds the 6 bytes from xa + 1 on (which run into the 5-byte Write): no
    other four-gram of those 6 lies inside one Write, so only the entry xa + 1 finds them.  back = 5:
    a copy of 6, candidate xa + 1.  back = 4: Go's candidate is whatever older position that bucket
    holds, refused, and the Write is one literal.  xa is at Write-relative position `lane` mod 32: 7 is
    an earlier lane of a 16- and of a 32-lane window, 15 the last of 16, 31 the last of both (back = 5:
    position xa + 1 is then another window's and its hash is computed anew)."""
    k = 10 - back
    b.fill(20)
    t = b.fill(10)
    b.fill(9)
    h = b.cut()
    b.fill(32 + (lane - (6 * k + 3)) % 32)
    for q in range(k):
        b.raw(b.collider(bytes(b.d[t + q : t + q + 4])))
        b.fill(1)
    b.fill(3)
    rep = b.copy(t, 10)
    b.avoid = None
    xa = rep + k
    n = b.cut() - h
    assert (xa - h) % 32 == lane and xa - h == n - back
    b.fill(5)
    h3 = b.cut()
    b.fill(7, avoid=(b.d[xa],))  # nothing found backward
    p = b.raw(bytes(b.d[xa + 1 : xa + 7]))
    b.avoid = b.d[xa + 7]
    b.fill(9)
    b.cut()
    b.want_at[1] = [lit(rep - h), cpy(10, rep - t)]
    b.must_at[1] = [("window", xa - h, t + k - h, rep - h, n)]
    b.want_at[2] = [lit(5)]
    c = xa + 1 - h3
    if back == 5:
        b.want_at[3] = [lit(7), cpy(6, p - (xa + 1)), lit(9)]
        b.must_at[3] = [("window", 7, c, 7, 13)]
    else:
        b.want_at[3] = [lit(22)]
        b.check_at[3] = [
            ("no older candidate refused at 7", lambda tr, c=c: any(e[0] == "short" and e[1] == 7 and e[2] < c for e in tr)),
            ("position xa + 1 is a candidate", lambda tr, c=c: not any(len(e) > 2 and e[2] == c for e in tr)),
        ]


def group_m2():
    cases = []
    for same in (False, True):
        br = "runlen" if same else "window"
        for j in M2_J:
            cases.append(make(f"M2-{br}-met-at-n-{4 + j}", lambda b, j=j, same=same: met_late(b, j, same), 1200 + 20 * same + j))
        cases.append(make(f"M2-{br}-met-only-at-n-3", lambda b, same=same: met_late(b, -1, same, 7), 1250 + same))
    for back in (5, 4):
        for lane in M2_LANES:
            cases.append(make(f"M2-insert-after-n-{back}-lane-{lane}", lambda b, back=back, lane=lane: extra_insert(b, back, lane), 1300 + 40 * back + lane))
    return cases


# ------------------------------------------------------------------ M3: Writes without a position

M3_LENS = (
    (0,), (0, 0), (1,), (3,), (0, 3), (3, 0), (1, 1, 1, 1), (3, 3, 3),
    (0, 40, 0), (40, 0, 0, 40), (2, 40), (40, 3, 40),
    (1,) * 64, (0,) * 8,
)  # fmt: skip


def short_writes(b: MSeq, lens):
    """Writes of the given lengths.  A Write of 40 bytes after another one of 40 is 7 bytes, 12 bytes
    that end 8 bytes before the other's end, and 21 bytes; every other Write is filler -- except that
    a stream of several Writes all under 4 bytes is periodic (period 1 for Writes of 1 byte, up to 4 of
    them; else period 3 or 8), so a parse that ignored the Writes' ends would find a run: a four-gram
    that straddles two Writes is never inserted and is never a candidate."""
    tiny = len(lens) > 1 and 0 < max(lens) < 4
    unit = bytes(b.rng.integers(1, 256, 1 if len(lens) == 4 else (3 if len(lens) == 3 else 8), dtype="uint8"))
    src = None
    for j, n in enumerate(lens):
        at = b.pos()
        if n == 40 and src is not None:
            b.fill(7)
            b.copy(src, 12)
            b.fill(21)
            b.want_at[j] = [lit(7), cpy(12, at + 7 - src), lit(21)]
            b.must_at[j] = [("window", 7, src - at, 7, 19)]
        else:
            if tiny:
                b.d += bytes(unit[(at + t) % len(unit)] for t in range(n))
            else:
                b.fill(n)
            b.want_at[j] = [lit(n)] if n else []
        if n == 40:
            src = b.pos() - 20
        b.cut()


def group_m3():
    return [make("M3-writes-of-" + ("-".join(map(str, lens)) if len(lens) < 8 else f"{len(lens)}x{lens[0]}"), lambda b, lens=lens: short_writes(b, lens), 1400 + j) for j, lens in enumerate(M3_LENS)]


# ------------------------------------------------------------------ M4: zeros at a boundary

M4_Z = (7, 8, 9, 16, 24, 25, 40)
M4_CUT = ((5, 5), (8, 8), (9, 9), (3, 20))
M4_AT_WEND = ((9, -1), (8, 0), (7, 1))  # (zeros that end the Write, cand + 8 - wend)


def zeros_end_tokens(pre: int, a: int):
    """Go's tokens and event of a Write of `pre` filler bytes and a zeros (writeRunlen :441-444: the
    zero token needs st + 8 < len(p)): the token from 9 on, a period-1 run of a - 1 for 7 and 8."""
    if a >= 9:
        return [lit(pre), cpy(a, 0)], [("zeros", pre + 1, pre, pre, pre + a)]
    if a >= 7:
        return [lit(pre + 1), cpy(a - 1, 1)], [("runlen", pre + 1, pre, pre + 1, pre + a)]
    return [lit(pre + a)], []


def zeros_start_tokens(avail, z: int, tail: int):
    """Go's tokens and first event of a Write that is z zeros and `tail` filler bytes when the zero
    four-gram's table entry lies `avail` bytes before the Write's first byte, in the zeros that end
    the Write before (None: no such entry).  The candidate is in the block, so this is the window
    branch, not the zero token: the forward count is trimmed to the bytes the block holds (trim 2),
    a copy of min(z, avail) at distance avail; the extra insert of position 1 makes the next
    candidate one byte nearer than this copy was long, and so on while 6 bytes are left of both.
    With fewer than 6 bytes available at position 0 that candidate is refused and position 1 finds
    position 0 in the Write itself: the zero token from 8 zeros on (st + 8 < len(p))."""
    toks, ev, i = [], [], 0
    while avail is not None and min(z - i, avail) >= 6:
        ln = min(z - i, avail)
        toks.append(cpy(ln, avail))
        ev.append(("window", i, i - avail, i, i + ln))
        i, avail = i + ln, ln - 1
    if i == 0 and z >= 8:
        return [cpy(z, 0), lit(tail)], [("zeros", 1, 0, 0, z)]
    assert z - i < 6, (z, i)
    return toks + [lit(z - i + tail)], ev[:1]


def zeros_at_end(b: MSeq, z: int):
    """z zeros that end a Write exactly; a Write of filler before and after."""
    b.fill(20)
    b.cut()
    b.fill(21)
    b.zeros(z)
    b.cut()
    b.fill(10)
    b.cut()
    b.want_at[1], b.must_at[1] = zeros_end_tokens(21, z)
    b.want_at[2] = [lit(10)]


def zeros_at_start(b: MSeq, z: int):
    """z zeros from a Write's first byte, after a Write that ends in 12 zeros (its zero token is
    accepted at the run's second byte, 11 bytes before its end: the table's entry)."""
    b.fill(20)
    b.zeros(12)
    b.cut()
    b.zeros(z)
    b.fill(12)
    b.cut()
    b.want_at[0] = [lit(20), cpy(12, 0)]
    b.want_at[1], b.must_at[1] = zeros_start_tokens(11, z, 12)


def zeros_cut(b: MSeq, a: int, c: int):
    """A run of a + c zeros cut by a Write boundary after a: each part is judged alone.  The entry the
    second part finds is the last zero four-gram the first part visited: its second byte when it was
    accepted there (a >= 7), else its position a - 4 (a >= 4)."""
    b.fill(20)
    b.cut()
    b.fill(21)
    b.zeros(a)
    b.cut()
    b.zeros(c)
    b.fill(12)
    b.cut()
    b.want_at[1], b.must_at[1] = zeros_end_tokens(21, a)
    b.want_at[2], b.must_at[2] = zeros_start_tokens(a - 1 if a >= 7 else (4 if a >= 4 else None), c, 12)


def group_m4():
    cases = [make(f"M4-{z}-zeros-end-the-Write", lambda b, z=z: zeros_at_end(b, z), 1500 + z) for z in M4_Z]
    cases += [make(f"M4-{z}-zeros-start-the-Write", lambda b, z=z: zeros_at_start(b, z), 1550 + z) for z in M4_Z]
    cases += [make(f"M4-zeros-cut-{a}+{c}", lambda b, a=a, c=c: zeros_cut(b, a, c), 1600 + a + c) for a, c in M4_CUT]
    # the zero-region guard cand + 8 < wend with zeros on the far side of the Write's end
    cases += [make(f"M4-candidate+8-at-wend{d:+d}", lambda b, a=a: zeros_cut(b, a, 8), 1650 + a) for a, d in M4_AT_WEND]
    return cases


# ------------------------------------------------------------------ M5: position 0 and the untouched table

M5_FIRST = ((12,), (40,), (3, 9), (1, 11))


def head_again(b: MSeq, first):
    """The stream's first 12 bytes again in a later Write, where nothing has taken their bucket since:
    the candidate is 0.  first = (12,) or (40,): position 0 was inserted; (3, 9) and (1, 11): its
    four-gram straddles two Writes and was never inserted, and still the zero table's entry points
    there."""
    for n in first:
        b.fill(n)
        b.cut()
    b.fill(25)
    h = b.cut()
    j = len(b.bounds)
    b.fill(7)
    x = b.raw(bytes(b.d[0:12]))
    b.avoid = b.d[12]
    b.fill(15)
    b.cut()
    b.want_at[j] = [lit(7), cpy(12, x), lit(15)]
    b.must_at[j] = [("window", 7, -h, 7, 19)]


def group_m5():
    return [make("M5-head-again-after-writes-of-" + "-".join(map(str, f)), lambda b, f=f: head_again(b, f), 1700 + j) for j, f in enumerate(M5_FIRST)]


# ------------------------------------------------------------------ M6: window lanes after a Write's start

M6_R = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)
M6_T = (0, 3, 4, 20)
M6_OFF = (1, 13, 16, 37)
# (r, t, the Write's stream offset): every r, every t, every offset; r + 10 + t is the Write's length
M6 = (
    (0, 0, 13), (0, 20, 37), (1, 3, 16), (1, 4, 13), (15, 0, 16), (15, 20, 1), (16, 3, 13), (16, 0, 1), (17, 4, 37),
    (31, 0, 13), (31, 3, 1), (32, 4, 16), (32, 20, 13), (33, 0, 37), (63, 3, 16), (63, 4, 1), (64, 20, 37), (64, 0, 16),
)  # fmt: skip


def lane_after_start(b: MSeq, r: int, t: int, off: int):
    """A second Write that starts at stream offset `off` and is r filler bytes, a 10-byte repeat and
    t filler bytes: k1_parse's windows restart at the Write's first byte, so the repeat is judged by
    lane r mod G of the window at r - r mod G, whose valid lanes end at the Write's position n - 4.
    off >= 13: the source lies in the first Write (the window branch).  off = 1: nothing can lie
    before the Write but one byte, so the source is the Write's first 10 bytes (run-length branch)."""
    if off >= 13:
        a = {13: 1, 16: 3, 37: 10}[off]
        b.fill(a)
        s = b.fill(10)
        b.fill(off - a - 10)
    else:
        b.fill(off)
    h = b.cut()
    assert h == off
    if off < 13:
        s = b.fill(10)
        b.fill(r - 10)
    else:
        b.fill(r)
    x = b.copy(s, 10)
    b.avoid = b.d[s + 10]
    b.fill(t)
    b.cut()
    b.want_at[1] = ([lit(r)] if r or off < 13 else []) + [cpy(10, x - s)] + ([lit(t)] if t else [])
    b.must_at[1] = [("window" if off >= 13 else "runlen", r, s - h, r, r + 10)]


def group_m6():
    return [make(f"M6-accept-at-{r}-tail-{t}-write-at-{off}", lambda b, r=r, t=t, off=off: lane_after_start(b, r, t, off), 1800 + 3 * r + t + off) for r, t, off in M6]


# ------------------------------------------------------------------ M7: the table limits

M7_T16 = 65536  # k1::kMaxT16: the longest stream the u16 table takes
M7_T32 = 1 << 19  # k1::kMaxT32: the 20-bit candidate field of k1_parse's `info`


def long_t16(b: MSeq, n: int):
    """n bytes in 3 Writes: 50 bytes that hold a 12-byte source, cheap history (Seq.bulk), and 60 bytes
    whose 12-byte repeat of the source is accepted at n - 15, among the last 16 visited positions."""
    b.fill(50)
    b.cut()
    b.bulk(n - 110)
    h = b.cut()
    b.fill(45)
    x = b.copy(20, 12)
    b.fill(3)
    assert b.cut() == n and x == n - 15
    b.want_at[2] = [lit(45), cpy(12, x - 20), lit(3)]
    b.must_at[2] = [("window", 45, 20 - h, 45, 57)]


def long_t32(b: MSeq, n: int):
    """n bytes in 3 Writes, the last one 50 bytes with a 12-byte source at n - 48 and its repeat at
    n - 28: candidate and acceptor above n - 64.  The stated tokens are the C oracle's alone."""
    b.fill(50)
    b.cut()
    b.bulk(n - 100)
    b.cut()
    b.fill(2)
    s = b.fill(12)
    b.fill(8)
    x = b.copy(s, 12)
    b.fill(16)
    assert b.cut() == n and s == n - 48 and x == n - 28
    b.want_at[2] = [lit(22), cpy(12, 20), lit(16)]
    b.c_only = True


def group_m7():
    """(the stream of 65,537 bytes has block 262,144: k1_parse takes a stream only in a block of twice
    its length, split_table_words, and the u32 table is chosen where the u16 one is too short)"""
    return [
        make("M7-65536-bytes-block-131072", lambda b: long_t16(b, M7_T16), 1900, 131072),
        make("M7-65537-bytes-block-262144", lambda b: long_t16(b, M7_T16 + 1), 1901, 262144),
        make("M7-2^19-bytes-block-1MiB", lambda b: long_t32(b, M7_T32), 1902, MiB),
        make("M7-2^19+1-bytes-block-1MiB", lambda b: long_t32(b, M7_T32 + 1), 1903, MiB),
    ]


M7_ROUTES = {
    "M7-65536-bytes-block-131072": "s:parse t16 mw",
    "M7-65537-bytes-block-262144": "s:parse t32 mw",
    "M7-2^19-bytes-block-1MiB": "s:parse t32 mw",
    "M7-2^19+1-bytes-block-1MiB": "w:view",
}


# ------------------------------------------------------------------ the handle's sequences as fresh streams

REUSED_GROUPS = ("R1", "R2", "R3", "R4", "R6")


@functools.lru_cache(maxsize=None)
def reused():
    """Every k1w_inputs case that sets no position (all of R1 - R4 and R6): its Writes are a fresh
    stream's Writes at the case's own block and table, where its parse was proved."""
    return tuple(c for g in REUSED_GROUPS for c in kw.group(g) if not c.pos)


def fits(c) -> bool:
    """Whether k1_parse takes the case's stream: 2n <= block (split_table_words) and n <= kMaxT16."""
    n = sum(len(p) for p in c.writes)
    return 2 * n <= c.block and n <= M7_T16


# ------------------------------------------------------------------ the groups, built once


@functools.lru_cache(maxsize=None)
def group(name: str):
    return tuple({"M1": group_m1, "M2": group_m2, "M3": group_m3, "M4": group_m4, "M5": group_m5, "M6": group_m6, "M7": group_m7}[name]())


GROUPS = ("M1", "M2", "M3", "M4", "M5", "M6", "M7")
SMALL = GROUPS[:-1]
