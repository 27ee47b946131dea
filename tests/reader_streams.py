"""Hand-built streams for the Reader handle's tests (eazy_amd/csrc/ez_reader.hip), host only.

A stream is written token by token (class Tokens, on k2_streams' lit / cpy / cpy_long / meta), which
keeps the intended token list and a plain model of the decode, so a case knows its tokens, its plain
bytes and where every buffer end falls before any decoder has seen it.  tests/test_gpu_reader_edges.py
proves those claims on the CPU (the oracle's walk, the oracle's decode, pyoracle's Reader) and then
holds the handle to the oracle Read by Read.

The three decode paths of the handle and how a case drives each:

  mode "s"  NewReader(io.Reader): the buffered input read ahead (stream_ahead, K2j continuing the
            stream).  ScriptSrc hands out the stream in scripted pieces, so the handle's buffer ends
            at the running sums (`cuts`) whatever capacities Reader._more works with; BufferSize is
            1 MiB so that no piece is clipped.  `aheads[j]` is the read-aheads buffer j must get.
  mode "w"  NewReaderBytes: the whole stream decoded at the first Read (reader_ahead); `whole` is what
            whole_decoded must say after it.  With `more`, a second part arrives through the Reader
            field once the first is served (ahead_leave).
  mode "r"  Read by Read (ez_reader_set_whole(h, 0)).  The handle would still read such a stream ahead
            (stream_ahead takes any handle that is not `whole` with 8 KiB buffered), so these streams
            are shorter than that or set SkipUnsupportedMeta, which declines it; `wins` are the upload
            windows' ends (65,536 bytes, or 2 * p_len + 64, from the Read's starting input position).

Constants the groups sit on (ez_reader.hip): kStreamMin = 8,192 buffered bytes for a read-ahead, the
slot 8 * n + 4096 and its 4x regrow, kAheadBrk = 65,536 Break positions, kStage = 4 MiB, the batch
choice K2t / K2j at 16 KiB of input, the 64 KiB upload window."""

from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle as orc
from k2_streams import HDR, HDR_1K, LIT, META_BREAK, META_MAGIC, META_RESET, META_VER, _E, _forms, cpy, cpy_long, lit, meta, rb

HDR_4K = b"\x80\x02eazy\x80\x10\x0c"  # magic, reset to a 4 KiB window
KiB, MiB = 1 << 10, 1 << 20
STREAM_MIN = 8 * KiB  # kStreamMin
STAGE = 4 * MiB  # kStage
BRK_CAP = 1 << 16  # kAheadBrk
WIN = 1 << 16  # the upload window of a Read by Read decode
BUFFER_SIZE = MiB  # BufferSize of every mode "s" case
LIMIT_S = 16 * MiB  # NewReader's BlockSizeLimit
META_UNSUP = 5 << 3  # a meta tag the format does not define

# kind: "l" literal, "c" copy, "m" meta, "z" a run of zero bytes (skipped, reader.go:221-223).
# start: the token's first byte in comp; hdr: its header bytes (a meta's or a zero run's whole length);
# L: output bytes; D: a copy's distance, a meta's tag; opos: plain bytes before it.
Tok = namedtuple("Tok", "kind start hdr L D opos")

Case = namedtuple("Case", "name group mode comp plain toks cuts where reads aheads whole more eof_after flags wins want split")
# where: for every cut (mode "s", the last one excepted when it is the stream's end) or window end
# (mode "r"), the (token index, byte of that token) it is meant to fall on; (index + 1, 0) is "exactly
# at token index's end".  want: ([(length, err) of every Read], their bytes joined), the oracle's.
# split: the first cut falls right after a meta's first byte.  The Reader has consumed that byte when it
# misses the second (continueMetaTag returns i, not st, reader.go:276-279), so the meta's second byte is
# read as a tag after the refill: the one place where a Read's result depends on where a refill falls.
# `want` is then the oracle's with its first refill ending at that cut, and plain is None.


def tok_end(t):
    return t.start + t.hdr + (t.L if t.kind == "l" else 0)


class Tokens:
    """A stream under construction: the bytes, the tokens meant, and the plain bytes they decode to
    (copies byte by byte, zeros before the window's first byte; None after a token that is an error)."""

    def __init__(self, rng, hdr=HDR):
        self.rng, self.c, self.toks, self.out, self.w0, self.bs = rng, bytearray(), [], bytearray(), 0, 0
        self.ok = True
        if hdr:
            self.meta(META_MAGIC, b"eazy")
            self.reset(hdr[-1])

    # -- positions
    @property
    def n(self):
        return len(self.c)

    @property
    def pos(self):
        """r.pos: plain bytes since the last MetaReset"""
        return len(self.out) - self.w0

    def _tok(self, kind, b, hdr, L, D):
        self.toks.append(Tok(kind, len(self.c), hdr, L, D, len(self.out)))
        self.c += b
        return len(self.toks) - 1

    # -- tokens
    def lit(self, n=None, body=None):
        body = rb(self.rng, n) if body is None else body
        b = lit(body)
        k = self._tok("l", b, len(b) - len(body), len(body), 0)
        self.out += body
        return k

    def cpy(self, D, L, long=False):
        b = cpy_long(D, L) if long else cpy(D, L)
        k = self._tok("c", b, len(b), L, D)
        if D > self.bs:
            self.ok = False  # ErrOverflow
        if D == 0:
            self.out += bytes(L)
        else:
            win = bytes(self.out[self.w0 :])[-D:]
            src = bytes(D - len(win)) + win
            self.out += (src * (L // D + 1))[:L]
        return k

    def meta(self, m, arg=b""):
        b = meta(m, arg)
        return self._tok("m", b, len(b), 0, m)

    def reset(self, bsl):
        k = self.meta(META_RESET, bytes([bsl]))
        self.w0, self.bs = len(self.out), 1 << bsl
        return k

    def brk(self):
        return self.meta(META_BREAK)

    def zeros(self, n):
        return self._tok("z", bytes(n), n, 0, 0)

    def raw(self, b):
        """bytes that are no whole token (a damaged tag, a truncated token): the stream's last"""
        self.c += b
        self.ok = False

    def form(self, b, hdr):
        """one of k2_streams._forms: a literal (hdr < len(b)), a copy or a meta, from its bytes"""
        tag, L, j, err = orc.dec_tag(b, 0)
        assert err == 0
        if tag == LIT:
            assert j == hdr
            return self.lit(body=b[hdr:])
        if L == 0:  # a meta
            m, ml, j2, err = orc.dec_meta(b, j)
            assert err == 0 and j2 + ml == len(b)
            return self.meta(m, b[j2:])
        D, j2, err = orc.dec_offset(b, j, L)
        assert err == 0 and j2 == len(b) == hdr
        k = self.cpy(D, L, long=b[j] == 0xFF and D >= L)
        assert bytes(self.c[-len(b) :]) == b
        return k

    def fill_to(self, target):
        """a literal that ends the stream so far at exactly `target` bytes"""
        e = _E()
        for tl in (1, 2, 3, 5):
            n = target - self.n - tl
            if n >= 1 and len(e.tag(b"", LIT, n)) == tl:
                k = self.lit(n)
                assert self.n == target
                return k
        raise AssertionError(("fill_to", self.n, target))

    def tail(self, n=STREAM_MIN + 600):
        """a short literal, a copy of it plus older bytes, and a literal of about n bytes: what follows
        a probe, so that a wrong byte or a wrong position shows in later bytes too"""
        self.lit(300)
        self.cpy(min(150, self.bs), 80)
        self.lit(n)
        self.cpy(min(700, self.bs), 40)
        self.lit(7)

    @property
    def plain(self):
        return bytes(self.out) if self.ok else None


# ---------------------------------------------------------------- the scripted io.Reader


class ScriptSrc:
    """An io.Reader that returns min(asked, pieces[j]) bytes at call j, EOF with the last bytes or
    (eof_after) at a call of its own after them.  It logs (asked, returned), the handle's read-ahead
    count and whole_decoded at every call, and refuses a call after it has said EOF with no bytes."""

    def __init__(self, comp, pieces, eof_after=False):
        assert sum(pieces) == len(comp) and all(p > 0 for p in pieces)
        self.b, self.pieces, self.eof_after = comp, list(pieces), eof_after
        self.at, self.log, self.counts, self.wholes, self.reader, self.ended = 0, [], [], [], None, False

    def read_go(self, k):
        import eazy_amd as ez

        assert not self.ended, "the source was asked again after EOF"
        self.counts.append(self.reader.ahead_count if self.reader is not None else 0)
        self.wholes.append(self.reader.whole_decoded if self.reader is not None else None)
        j = len(self.log)
        if j >= len(self.pieces):
            self.ended = True
            self.log.append((k, 0))
            return b"", ez.EOF
        m = min(k, self.pieces[j])
        d = self.b[self.at : self.at + m]
        self.at += m
        self.log.append((k, m))
        return d, (ez.EOF if j == len(self.pieces) - 1 and not self.eof_after else ez.OK)

    @property
    def sums(self):
        return tuple(int(x) for x in np.cumsum([m for _, m in self.log if m]))


# ---------------------------------------------------------------- Reads and the oracle's answer


def run_reads(read, sizes, max_reads=400_000):
    """Read with the given sizes (the last one repeated) until an error other than ErrBreak."""
    out = []
    while len(out) < max_reads:
        d, err = read(sizes[min(len(out), len(sizes) - 1)])
        out.append((bytes(d), err))
        if err not in (orc.OK, orc.EBREAK):
            break
    return out


def pack(reads, plain=None):
    data = b"".join(d for d, _ in reads)
    return [(len(d), e) for d, e in reads], (plain if plain is not None and data == plain else data)


def oracle_reader(mode, comp, more=None, eof_after=False, flags=(False, False), first=None):
    """the C oracle's Reader for a case: NewReader over the stream in one piece (chunk 0; Read's results
    do not depend on where refills fall, with the one exception `first` is for: its first refill then
    ends at that byte, BufferSize being that much), or NewReaderBytes"""
    if mode == "s" or more is not None:
        r = orc.Reader(src=comp + (more or b""), eof_with_data=not eof_after, chunk=0)
        r.set(LIMIT_S if mode == "s" else 0, first or BUFFER_SIZE, *flags)
    else:
        r = orc.Reader(b=comp)
        r.set(0, 0, *flags)
    return r


def make(name, group, mode, t, cuts=(), where=(), reads=(4096,), aheads=(), whole=None, more=None, eof_after=False,
         flags=(False, False), wins=(), comp=None, plain="model"):
    comp = bytes(t.c) if comp is None else comp
    plain = t.plain if plain == "model" else plain
    if mode == "s":
        cuts = tuple(cuts) + ((len(comp),) if not cuts or cuts[-1] != len(comp) else ())
        assert all(a < b for a, b in zip((0,) + cuts, cuts)), (name, cuts)
        assert len(aheads) == len(cuts), (name, aheads, cuts)
    want = pack(run_reads(oracle_reader(mode, comp, more, eof_after, flags).read, reads), plain)
    split = False
    if mode == "s" and len(cuts) > 1:
        w2 = pack(run_reads(oracle_reader(mode, comp, more, eof_after, flags, first=cuts[0]).read, reads), plain)
        if w2 != want:
            k, off = where[0]
            _need(off == 1 and t.toks[k].kind == "m", name, "a Read's result depends on the refill")
            split, plain, want = True, None, pack(run_reads(oracle_reader(mode, comp, more, eof_after, flags, first=cuts[0]).read, reads))
            # (buffer 2 is then other tokens than the ones meant: handed over if they end in an error of
            # the format, read ahead if they just end inside one)
            aheads = (aheads[0], int(want[0][-1][1] in (orc.EOF, orc.EUNEXPECTEDEOF)))
    return Case(name, group, mode, comp, plain, tuple(t.toks), tuple(cuts), tuple(where), tuple(reads), tuple(aheads), whole,
                more, eof_after, tuple(flags), tuple(wins), want, split)


def _need(cond, *what):
    if not cond:
        raise AssertionError(("the builder cannot make this case",) + what)


# ---------------------------------------------------------------- S1 / R1: a buffer end inside every form

FORMS = ("lit_len0", "lit_len1", "lit_len2", "lit_len4", "cpy_plain", "cpy_off1", "cpy_off2", "cpy_len1_off1", "cpy_len2",
         "cpy_off4", "cpy_len4_run", "cpy_long", "zero_region", "break", "ver", "magic")


def forms(rng):
    f = {name: (b, hdr, far) for name, b, hdr, far in _forms(rng)}
    return [(name,) + f[name] for name in FORMS]


def form_cuts(b, hdr):
    """the bytes of a form a buffer end is placed on: its start, after each header byte but the last,
    its end; for a literal also right after the header, after 1 body byte, at half the body and at
    the body less 1"""
    xs = list(range(hdr)) + [len(b)]
    if len(b) > hdr:
        body = len(b) - hdr
        xs += [hdr, hdr + 1, hdr + body // 2, hdr + body - 1]
    return sorted(set(xs))


def _far_history(t):
    """70,300 bytes of output from 305 bytes of input (a random literal repeated): room for cpy_off4"""
    t.lit(300)
    t.cpy(300, 70_000)


@lru_cache(None)
def s1_cases():
    """Streams of 20 to 40 KiB (lit_len4: 90 KiB, its body is 70,000 bytes): a 9,000-byte literal, the
    form, a tail of 9,500 bytes.  Buffer 1 ends on the chosen byte of the form; buffer 2 starts where
    the form started (the cut is in its header), at the cut (it is at the form's start or end, or in a
    literal's body).  Both buffers are read ahead."""
    out = []
    rng = np.random.default_rng(2101)
    for name, b, hdr, far in forms(rng):
        for x in form_cuts(b, hdr):
            t = Tokens(rng)
            if far:
                _far_history(t)
            t.lit(9000)
            k = t.form(b, hdr)
            T = t.toks[k].start
            t.tail()
            where = (k + 1, 0) if x == len(b) else (k, x)
            out.append(make(f"s1-{name}-x{x}", "S1", "s", t, cuts=(T + x,), where=(where,), aheads=(1, 1), reads=(4096,)))
    return out


def _read_start(t, p_len):
    """the input position at the start of the Read of p_len bytes that takes the last plain byte so
    far: inside a literal's body, after a copy's token (its bytes come from the window), or 0"""
    at = (len(t.out) - 1) // p_len * p_len
    if at == 0:
        return 0
    for k in t.toks:
        if k.kind in "lc" and k.opos <= at < k.opos + k.L:
            if at == k.opos:
                return k.start
            return k.start + k.hdr + (at - k.opos if k.kind == "l" else 0)
    raise AssertionError(at)


@lru_cache(None)
def r1_cases():
    """A zero run (skipped input that makes no output) up to the form, so that the upload window of the
    Read that reaches it, 65,536 bytes from that Read's starting input position (byte 0 but for
    cpy_off4, whose history takes Reads of its own), ends on the chosen byte of the form; for every
    form also one Read of 40,000 bytes, whose window is 2 * 40,000 + 64 bytes.  SkipUnsupportedMeta
    is on: it declines the read-ahead and changes no result (no stream has such a meta)."""
    out = []
    rng = np.random.default_rng(2102)
    for name, b, hdr, far in forms(rng):
        # (a literal's body is output: the Read must hold what comes before the window's end, so
        # lit_len4's 70,000 bytes take Reads of 80,000 bytes and their window of 160,064)
        p0 = 80_000 if name == "lit_len4" else 4096
        for win, p_len, xs in ((max(WIN, 2 * p0 + 64), p0, form_cuts(b, hdr)), (2 * 40_000 + 64, 40_000, [1 if hdr > 1 else 0])):
            for x in xs:
                t = Tokens(rng)
                if far:
                    _far_history(t)
                t.lit(800)
                end = _read_start(t, p_len) + win  # the window of the Read that takes the literal's last byte
                _need(end - x - t.n > 0, name, x)
                t.zeros(end - x - t.n)
                k = t.form(b, hdr)
                _need(t.toks[k].start + x == end, name, x)
                t.tail(400)
                where = (k + 1, 0) if x == len(b) else (k, x)
                out.append(make(f"r1-{name}-w{win}-x{x}", "R1", "r", t, wins=(end,), where=(where,), reads=(p_len,),
                                flags=(False, True), aheads=()))
    return out


# ---------------------------------------------------------------- S2: the pending literal

S2_K = (1, 15, 16, 17, 8191, 8192)


def _s2_probe(t, k, kind):
    """the first token after the k pending bytes"""
    if kind == "in-pending":
        t.cpy(k, min(k, 30))
    elif kind == "in-history":
        t.cpy(k + 100, 50)
    elif kind == "seam-history-pending":
        t.cpy(k + 10, 10 + min(k, 10))
    elif kind == "seam-pending-output":
        t.cpy(min(k, 5), 40)
    elif kind == "run1":
        t.cpy(1, 100)
    else:
        raise AssertionError(kind)


@lru_cache(None)
def s2_cases():
    """A literal spans the first cut with k bytes of it in buffer 2 (stream_ahead puts them in front of
    K2j's output: c_hist = H + k, c_pos0 = pos + k, Break positions move by k).  Then a copy whose source
    lies in the pending bytes, in the history before them, across either seam, or a distance-1 run that
    starts on the last pending byte.  Two more: the literal's rest is all of buffer 2 (n2 == 0, the
    state returns to 0) and more than buffer 2 (n2 == 0, the state stays 'l': three buffers)."""
    out = []
    rng = np.random.default_rng(2103)
    for k in S2_K:
        for kind in ("in-pending", "in-history", "seam-history-pending", "seam-pending-output", "run1"):
            t = Tokens(rng)
            t.lit(8500)
            j = t.lit(600 + k)
            cut = tok_end(t.toks[j]) - k
            _s2_probe(t, k, kind)
            t.tail()
            out.append(make(f"s2-k{k}-{kind}", "S2", "s", t, cuts=(cut,), where=((j, cut - t.toks[j].start),), aheads=(1, 1)))
    for name, nbuf in (("rest-is-buffer-2", 1), ("rest-exceeds-buffer-2", 2)):
        t = Tokens(rng)
        t.lit(8500)
        j = t.lit(600 + nbuf * 9000)
        end = tok_end(t.toks[j])
        cuts = tuple(end - q * 9000 for q in range(nbuf, -1, -1))
        t.cpy(9000, 60)
        t.tail()
        out.append(make(f"s2-{name}", "S2", "s", t, cuts=cuts, where=tuple((j, c - t.toks[j].start) if c < end else (j + 1, 0) for c in cuts),
                        aheads=(1,) * (len(cuts) + 1)))
    return out


# ---------------------------------------------------------------- S3: the history seam and the window's edges


def _s3_first(t, pos):
    """output up to `pos` in well under 8 KiB of input: a random literal and copies of it"""
    n = min(pos, 600)
    t.lit(n)
    while t.pos < pos:
        L = min(pos - t.pos, 333)
        t.cpy(min(t.pos, t.bs, 257), L)


@lru_cache(None)
def s3_cases():
    """Windows of 1 KiB and 4 KiB.  Buffer 1 is short (decoded Read by Read: the read-ahead takes the
    window and position the exact decoder left) and ends with pos at bs - 1, bs, bs + 1, 2 * bs + 5 or
    100; buffer 2 is read ahead and starts with a copy that reaches the oldest history byte exactly,
    then one at distance bs exactly; in a case of its own distance bs + 1 (ErrOverflow, at the
    oracle's Read; handed over), and with pos = 100 a distance of 500 (before the stream's first byte).
    Sixteen more under the 1 MiB window: the same tokens, the literal before the cut 0 to 15 bytes
    longer, both buffers read ahead, so the read-ahead's output starts at every residue mod 16."""
    out = []
    rng = np.random.default_rng(2104)
    for wname, hdr in (("1k", HDR_1K), ("4k", HDR_4K)):
        bs = 1 << hdr[-1]
        for pname, pos in (("bs-1", bs - 1), ("bs", bs), ("bs+1", bs + 1), ("2bs+5", 2 * bs + 5), ("100", 100)):
            for probe in ("oldest-and-bs", "bs+1") + (("before-start",) if pos == 100 else ()):
                t = Tokens(rng, hdr)
                _s3_first(t, pos)
                cut = t.n
                _need(cut < STREAM_MIN and t.pos == pos, wname, pname)
                if probe == "oldest-and-bs":
                    t.cpy(min(pos, bs), 37)
                    t.lit(11)
                    t.cpy(bs, 90)
                elif probe == "bs+1":
                    t.lit(5)
                    t.cpy(bs + 1, 20)
                else:
                    t.cpy(500, 120)
                    t.lit(3)
                    t.cpy(700, 900)  # (overlapping: zero bytes, the stream's first bytes, and both again)
                t.tail()
                out.append(make(f"s3-{wname}-pos-{pname}-{probe}", "S3", "s", t, cuts=(cut,), where=((len([x for x in t.toks if x.start < cut]), 0),),
                                aheads=(0, 0 if probe == "bs+1" else 1)))
    for extra in range(16):
        t = Tokens(rng)
        t.lit(9000 + extra)
        cut = t.n
        k = t.cpy(9000 + extra, 33)
        t.cpy(16, 50)
        t.tail()
        out.append(make(f"s3-residue-{extra}", "S3", "s", t, cuts=(cut,), where=((k, 0),), aheads=(1, 1)))
    return out


# ---------------------------------------------------------------- S4 / S7: slot growth


def _s4_stream(rng, n2, out_n, dist, tail_lit=0):
    """buffer 1 (a 9,000-byte literal, read ahead), then exactly n2 bytes of input that decode to exactly
    out_n bytes: a literal and one long copy at distance `dist` (0: a zero region); with tail_lit, the
    input's last bytes are a literal's header and the first tail_lit bytes of its body (they count in
    out_n), and the body's rest is buffer 3."""
    t = Tokens(rng)
    t.lit(9000)
    cut, first = t.n, len(t.toks)
    e = _E()
    th = e.tag(b"", LIT, tail_lit + 9000) if tail_lit else b""
    fixed = len(th) + tail_lit
    for ch in range(2, 9):  # the copy token's length
        for lh in (1, 2, 3, 5):  # the literal's header
            ll = n2 - fixed - ch - lh
            L = out_n - tail_lit - ll
            if ll >= 1 and L >= 1 and len(e.tag(b"", LIT, ll)) == lh and len(cpy(dist, L)) == ch:
                t.lit(ll)
                t.cpy(dist, L)
                if tail_lit:
                    j = t.lit(tail_lit + 9000)
                    cut2 = t.toks[j].start + t.toks[j].hdr + tail_lit
                    t.tail()
                    _need(cut2 - cut == n2 and t.toks[j].opos + tail_lit - 9000 == out_n)
                    return t, (cut, cut2), ((first, 0), (j, cut2 - t.toks[j].start))
                _need(t.n - cut == n2 and len(t.out) - 9000 == out_n)
                return t, (cut,), ((first, 0),)
    raise AssertionError(("the builder cannot make this case", n2, out_n))


S7_N2 = 65_600  # 16 * (8 * n2 + 4096) = 8,462,336: two regrows hold a little over 8 MiB
S7_OUT = 8 * MiB + 4196


@lru_cache(None)
def s4_cases():
    """Buffer 2 is n2 = 8,192 bytes of input whose output is exactly 8 * n2 + 4096 bytes (the slot), one
    more (one 4x regrow), 200,000 (one regrow), and, with n2 = 65,600, a little over 8 MiB (two regrows;
    S7 serves the same stream); twice the input ends in a cut literal whose bytes there are bring the
    output to exactly the slot and to one more."""
    rng = np.random.default_rng(2105)
    n2 = STREAM_MIN
    cap = 8 * n2 + 4096
    out = []
    for name, a in (("slot-exact", (n2, cap, 1)), ("slot-plus1", (n2, cap + 1, 0)), ("regrow-once", (n2, 200_000, 1)),
                    ("tail-slot-exact", (n2, cap, 1, 700)), ("tail-slot-plus1", (n2, cap + 1, 0, 700)),
                    ("regrow-twice-8mib", (S7_N2, S7_OUT, 1))):
        t, cuts, where = _s4_stream(rng, *a)
        out.append(make(f"s4-{name}", "S4", "s", t, cuts=cuts, where=where, aheads=(1,) * (len(cuts) + 1), reads=(65536,)))
    return out


def stage_reads():
    """Read sizes round the 4 MiB staging window of a read-ahead of a little over 8 MiB"""
    return (("stage-1", (STAGE - 1,)), ("stage", (STAGE,)), ("stage+1", (STAGE + 1,)), ("direct-from-mid-window", (MiB, 7 * MiB + 5, 65536)),
            ("4k-end-before", (STAGE - 4097, 4096)), ("4k-end-on", (STAGE - 4096, 4096)), ("4k-end-across", (STAGE - 4095, 4096)))


@lru_cache(None)
def s7_cases():
    """S4's largest stream (buffer 2 decodes to a little over 8 MiB) with Reads round the staging
    window.  The first 9,000 bytes served are buffer 1's; the window's edges are counted from buffer
    2's first byte, so the first Read takes buffer 1's bytes."""
    out = []
    for name, sizes in stage_reads():
        c = s4_cases()[-1]._replace(name=f"s7-{name}", group="S7", reads=(9000,) + sizes)
        want = pack(run_reads(oracle_reader("s", c.comp).read, c.reads), c.plain)
        out.append(c._replace(want=want))
    return out


@lru_cache(None)
def w3_cases():
    """The same tokens as S7's buffer 2 as one NewReaderBytes stream (reader_ahead, K2j, two regrows)"""
    rng = np.random.default_rng(2106)
    t = Tokens(rng)
    t.lit(S7_N2 - 9 - 5 - 7)
    t.cpy(1, S7_OUT - len(t.out))
    return [make(f"w3-{name}", "W3", "w", t, whole=True, reads=sizes) for name, sizes in stage_reads()]


# ---------------------------------------------------------------- S5 / W2: Breaks


BRK_READS = (("end-before", -1), ("end-on", 0), ("end-past", 1))  # the first Read's end against the Break's plain position


def _s5_layout(rng, place):
    """(tokens, cuts, where, plain position of the first Break placed)"""
    t = Tokens(rng)
    if place == "first-in-buffer":
        t.lit(9000)
        cut = t.n
        k = t.brk()
        t.tail()
        return t, (cut,), ((k, 0),), t.toks[k].opos
    if place == "after-pending":
        t.lit(8500)
        j = t.lit(900)
        cut = tok_end(t.toks[j]) - 77  # k = 77
        k = t.brk()
        t.tail()
        return t, (cut,), ((j, cut - t.toks[j].start),), t.toks[k].opos
    if place in ("last-whole-token", "three-in-a-row"):
        t.lit(9000)
        t.cpy(40, 25)
        k = t.brk()
        if place == "three-in-a-row":
            t.brk()
            t.brk()
            cut = t.n
            t.tail()
            return t, (cut,), ((k + 3, 0),), t.toks[k].opos
        j = t.cpy(320, 20)  # its 3 bytes split 1 / 2 by the cut: the Break is the last whole token
        t.tail()
        return t, (t.toks[j].start + 1,), ((j, 1),), t.toks[k].opos
    if place == "split":
        t.lit(9000)
        t.cpy(40, 25)
        k = t.brk()
        t.tail()
        return t, (t.toks[k].start + 1,), ((k, 1),), t.toks[k].opos
    raise AssertionError(place)


S5_PLACES = ("first-in-buffer", "after-pending", "last-whole-token", "three-in-a-row", "split")


@lru_cache(None)
def s5_cases():
    out = []
    rng = np.random.default_rng(2107)
    for place in S5_PLACES:
        for rname, d in BRK_READS:
            t, cuts, where, at = _s5_layout(rng, place)
            out.append(make(f"s5-{place}-{rname}", "S5", "s", t, cuts=cuts, where=where, aheads=(1, 1), reads=(at + d, 4096)))
    return out


def _many_breaks(t, n):
    """n Breaks, a 1-byte literal after every 1,024th"""
    for q in range(n):
        t.brk()
        if q % 1024 == 1023:
            t.lit(1)


@lru_cache(None)
def s5_cap_cases():
    """65,536 Breaks in buffer 2 (served from the read-ahead) and 65,537 (handed over: no read-ahead
    for that buffer); 131 KiB of input each"""
    out = []
    rng = np.random.default_rng(2108)
    for n, ahead in ((BRK_CAP, 1), (BRK_CAP + 1, 0)):
        t = Tokens(rng)
        t.lit(9000)
        cut = t.n
        _many_breaks(t, n)
        t.lit(50)
        out.append(make(f"s5-breaks-{n}", "S5cap", "s", t, cuts=(cut,), where=((3, 0),), aheads=(1, ahead), reads=(64,)))
    return out


@lru_cache(None)
def w2_cases():
    """S5's placements as NewReaderBytes streams (the buffer ends play no part: a Break first, after a
    literal and a copy, last in the stream, three in a row), each with the first Read ending one byte
    before the Break, on it and one past it; all decoded whole."""
    out = []
    rng = np.random.default_rng(2109)
    for place in ("first", "after-literal", "last", "three-in-a-row"):
        for rname, d in BRK_READS:
            t = Tokens(rng)
            if place != "first":
                t.lit(5000)
                t.cpy(40, 25)
            k = t.brk()
            if place == "three-in-a-row":
                t.brk()
                t.brk()
            if place != "last":
                t.tail(3000)
            at = t.toks[k].opos
            out.append(make(f"w2-{place}-{rname}", "W2", "w", t, whole=True, reads=(max(at + d, 1), 4096)))
    return out


@lru_cache(None)
def w2_cap_cases():
    """65,536 Breaks (decoded whole) and 65,537 (whole_decoded false: Read by Read); the same bytes and
    errors either way"""
    out = []
    rng = np.random.default_rng(2110)
    for n in (BRK_CAP, BRK_CAP + 1):
        t = Tokens(rng)
        t.lit(100)
        _many_breaks(t, n)
        t.lit(50)
        out.append(make(f"w2-breaks-{n}", "W2cap", "w", t, whole=n <= BRK_CAP, reads=(64,)))
    return out


# ---------------------------------------------------------------- S6: declines and hand-overs


@lru_cache(None)
def s6_cases():
    out = []
    rng = np.random.default_rng(2111)
    # 8,191 / 8,192 bytes buffered
    for n in (STREAM_MIN - 1, STREAM_MIN):
        t = Tokens(rng)
        t.lit(3000)
        t.cpy(100, 60)
        t.fill_to(n)
        out.append(make(f"s6-buffered-{n}", "S6", "s", t, aheads=(int(n >= STREAM_MIN),)))
    # a MetaReset after output in buffer 2 (handed over); buffer 3 is read ahead again
    t = Tokens(rng)
    t.lit(9000)
    c1 = t.n
    t.lit(4000)
    k = t.reset(12)
    t.lit(5000)
    t.cpy(4096, 30)
    c2 = t.n
    j = t.cpy(200, 50)
    t.tail()
    out.append(make("s6-reset-after-output", "S6", "s", t, cuts=(c1, c2), where=((3, 0), (j, 0)), aheads=(1, 0, 1)))
    # in buffer 2, after a buffer that was read ahead: a distance past the window, a damaged tag, an
    # unsupported meta -- the oracle's error at the oracle's Read
    for name in ("distance-past-window", "damaged-tag", "unsupported-meta"):
        t = Tokens(rng, HDR_1K)
        t.lit(9000)
        c1 = t.n
        t.lit(4500)
        t.cpy(1024, 30)
        if name == "distance-past-window":
            t.cpy(1025, 30)
            t.tail()
        elif name == "unsupported-meta":
            t.meta(META_UNSUP, b"ab")
            t.ok = False
            t.tail()
        else:
            t.raw(b"\x7f" + rb(rng, STREAM_MIN))
        out.append(make(f"s6-{name}", "S6", "s", t, cuts=(c1,), where=((3, 0),), aheads=(1, 0)))
    # RequireMagic and SkipUnsupportedMeta: no read-ahead
    for name, flags in (("require-magic", (True, False)), ("skip-unsupported-meta", (False, True))):
        t = Tokens(rng)
        t.lit(9000)
        c1 = t.n
        t.cpy(500, 44)
        if flags[1]:
            t.meta(META_UNSUP, b"ab")
        t.tail()
        out.append(make(f"s6-{name}", "S6", "s", t, cuts=(c1,), where=((3, 0),), aheads=(0, 0), flags=flags))
    # a Read that fills p in the middle of a copy, then a refill: buffer 1 is short (Read by Read), its
    # last token a copy that the Reads of 100 bytes leave half served when the input runs out
    t = Tokens(rng)
    t.lit(3000)
    t.cpy(2000, 950)
    c1 = t.n
    t.tail()
    out.append(make("s6-p-full-mid-copy-then-refill", "S6", "s", t, cuts=(c1,), where=((len(t.toks) - 5, 0),), aheads=(0, 1), reads=(100,) * 35 + (4096,)))
    return out


@lru_cache(None)
def s6_ver_cases():
    """Three streams for one handle in turn.  A: a MetaVer with version 1 (ErrUnsupportedVersion; no
    read-ahead).  B: a clean two-buffer stream after Reset: the Reader keeps the version, so still no
    read-ahead.  C: a MetaVer 0, then a 5,000-byte copy that Reads of 4,096 bytes leave half served
    with 9 KiB still buffered: the exact decoder takes the first Read (the version was 1), the second
    finds the handle mid-copy (stream_ahead's state == 'c' guard: the only way to it, the read-ahead
    being tried at every Read but declined for good by every other reason), the third reads ahead from
    inside a literal."""
    rng = np.random.default_rng(2118)
    a = Tokens(rng)
    a.meta(META_VER, b"\x01")
    a.ok = False
    a.lit(9000)
    a.tail()
    b = Tokens(rng)
    b.lit(9000)
    c1 = b.n
    b.cpy(500, 44)
    b.tail()
    c = Tokens(rng)
    c.lit(200)
    c.meta(META_VER, b"\x00")
    c.cpy(100, 5000)
    c.tail(12_000)
    return [make("s6-version-1", "S6ver", "s", a, aheads=(0,)),
            make("s6-version-kept", "S6ver", "s", b, cuts=(c1,), where=((3, 0),), aheads=(0, 0)),
            make("s6-version-0-mid-copy", "S6ver", "s", c, aheads=(1,))]


@lru_cache(None)
def s6_eof_cases():
    """The stream ends inside each form (half way through the header, and for a literal half way through
    the body too), with EOF arriving with the last bytes and at a call of its own after them: the bytes
    there are first, then io.ErrUnexpectedEOF, as the oracle says.  One buffer, read ahead."""
    out = []
    rng = np.random.default_rng(2112)
    for name, b, hdr, far in forms(rng):
        xs = ([hdr // 2] if hdr > 1 else []) + ([hdr, hdr + (len(b) - hdr) // 2] if len(b) > hdr else [])
        for x in xs:
            for eof_after in (False, True):
                t = Tokens(rng)
                if far:
                    _far_history(t)
                t.lit(9000)
                t.cpy(77, 20)
                t.raw(b[:x])
                # (a meta's first byte alone is consumed before its second is missed, reader.go:272-280:
                # nothing is left over and the stream ends with a clean EOF)
                t.ok = b[:x] == b"\x80"
                out.append(make(f"s6-eof-in-{name}-x{x}-{'after' if eof_after else 'with'}", "S6eof", "s", t, aheads=(1,),
                                eof_after=eof_after))
    for eof_after in (False, True):  # zero padding is consumed as it is skipped: a clean EOF
        t = Tokens(rng)
        t.lit(9000)
        t.cpy(77, 20)
        t.zeros(5)
        out.append(make(f"s6-eof-after-zero-padding-{'after' if eof_after else 'with'}", "S6eof", "s", t, aheads=(1,), eof_after=eof_after))
    return out


# ---------------------------------------------------------------- W1 / W5: whole decode, K2t and K2j


@lru_cache(None)
def w1_cases():
    """b_len 16,383 (K2t), 16,384 and 16,385 (K2j), the same token forms: a literal and one distance-1
    run that brings the output to exactly 8 * b_len + 4096 (the slot), one more (one regrow) and
    600,000 bytes (two).  In this order one handle runs them small, large, small (W5)."""
    out = []
    rng = np.random.default_rng(2113)
    for n in (16_383, 16_384, 16_385):
        for name, out_n in (("slot-exact", 8 * n + 4096), ("regrow-twice", 600_000), ("slot-plus1", 8 * n + 4097)):
            t = None
            for ch in range(2, 9):
                for lh in (1, 2, 3, 5):
                    ll = n - 9 - ch - lh
                    L = out_n - ll
                    if t is None and len(_E().tag(b"", LIT, ll)) == lh and len(cpy(1, L)) == ch:
                        t = Tokens(rng)
                        t.lit(ll)
                        t.cpy(1, L)
            _need(t is not None and t.n == n and len(t.out) == out_n, n, name)
            out.append(make(f"w1-blen{n}-{name}", "W1", "w", t, whole=True, reads=(65536,)))
    return out


# ---------------------------------------------------------------- W4: input after the decoded stream


@lru_cache(None)
def w4_cases():
    """A NewReaderBytes stream decoded whole and served, then more input through the Reader field
    (ahead_leave: Read by Read from the window, position and history at the stream's end).  The end
    position is bs - 1, bs, bs + 1 and 2 * bs + 5 under windows of 1 KiB and 4 KiB; the new input starts
    with a copy that reaches the oldest history byte, then one at distance bs.  One stream is the magic
    alone (no MetaReset: end_bs == 0); the new input brings the MetaReset."""
    out = []
    rng = np.random.default_rng(2114)
    for wname, hdr in (("1k", HDR_1K), ("4k", HDR_4K)):
        bs = 1 << hdr[-1]
        for pname, pos in (("bs-1", bs - 1), ("bs", bs), ("bs+1", bs + 1), ("2bs+5", 2 * bs + 5)):
            t = Tokens(rng, hdr)
            _s3_first(t, pos)
            n1 = t.n
            t.cpy(min(pos, bs), 37)
            t.lit(11)
            t.cpy(bs, 90)
            t.tail(500)
            c = bytes(t.c)
            out.append(make(f"w4-{wname}-end-{pname}", "W4", "w", t, whole=True, comp=c[:n1], more=c[n1:], reads=(300,)))
    t = Tokens(rng, None)
    t.meta(META_MAGIC, b"eazy")
    n1 = t.n
    t.reset(10)
    t.lit(700)
    t.cpy(700, 50)
    t.tail(500)
    c = bytes(t.c)
    out.append(make("w4-no-reset", "W4", "w", t, whole=True, comp=c[:n1], more=c[n1:], reads=(300,)))
    return out


# ---------------------------------------------------------------- R2 - R4: Read by Read


def _r2_stream(rng):
    t = Tokens(rng, HDR_1K)
    t.lit(40)
    t.cpy(25, 18)
    t.cpy(0, 30)
    t.lit(9)
    t.cpy(3, 20)
    t.brk()
    t.lit(130)
    t.cpy(1, 17)
    t.cpy(100, 12, long=True)
    t.lit(4)
    return t


@lru_cache(None)
def r2_cases():
    """One short stream.  p ends exactly at a token's end, one byte before it, inside a copy, inside a
    literal and inside a zero region, each followed by Reads that continue; and p_len 1 throughout."""
    rng = np.random.default_rng(2115)
    out = []
    ends = (("token-end", 40 + 18), ("token-end-less-1", 40 + 17), ("in-copy", 40 + 7), ("in-literal", 23), ("in-zero-region", 40 + 18 + 11))
    for name, first in ends + (("plen-1", 1),):
        t = _r2_stream(np.random.default_rng(2115))
        out.append(make(f"r2-{name}", "R2", "r", t, reads=(first, 1, 2, 50) if first > 1 else (1,)))
    del rng
    return out


@lru_cache(None)
def r3_cases():
    """The history's hand-over between the two decode buffers with pos at bs - 1, bs and bs + 1 at a
    Read's end (windows of 1 KiB and 4 KiB), then a Read 100 times larger than any before it
    (grow_keep_history must keep the history: the first token of that Read copies the oldest byte).
    Under 8 KiB of input: copies of a random literal make the output."""
    out = []
    rng = np.random.default_rng(2116)
    for wname, hdr in (("1k", HDR_1K), ("4k", HDR_4K)):
        bs = 1 << hdr[-1]
        for pname, pos in (("bs-1", bs - 1), ("bs", bs), ("bs+1", bs + 1)):
            t = Tokens(rng, hdr)
            _s3_first(t, pos)
            t.cpy(min(pos, bs), 37)
            t.lit(11)
            t.cpy(bs, 90)
            while len(t.out) < 101 * pos:
                t.cpy(int(rng.integers(1, bs + 1)), int(rng.integers(200, 3000)))
            t.lit(5)
            _need(t.n < STREAM_MIN, wname, pname, t.n)
            out.append(make(f"r3-{wname}-pos-{pname}", "R3", "r", t, reads=(pos, 100 * pos, 4096)))
    return out


@lru_cache(None)
def r4_cases():
    """A skipped meta (SkipUnsupportedMeta) whose body is longer than the upload window: the decoder
    makes no progress until the window holds the whole meta, so the window doubles (once for a
    70,000-byte body, twice for 140,000)."""
    out = []
    rng = np.random.default_rng(2117)
    for n in (70_000, 140_000):
        t = Tokens(rng)
        t.lit(500)
        t.meta(META_UNSUP, rb(rng, n))
        t.cpy(500, 60)
        t.tail(400)
        out.append(make(f"r4-skipped-meta-{n}", "R4", "r", t, reads=(4096,), flags=(False, True)))
    return out


# ---------------------------------------------------------------- all groups

GROUPS = {"S1": s1_cases, "S2": s2_cases, "S3": s3_cases, "S4": s4_cases, "S5": s5_cases, "S5cap": s5_cap_cases, "S6": s6_cases,
          "S6eof": s6_eof_cases, "S6ver": s6_ver_cases, "S7": s7_cases, "W1": w1_cases, "W2": w2_cases, "W2cap": w2_cap_cases, "W3": w3_cases, "W4": w4_cases,
          "R1": r1_cases, "R2": r2_cases, "R3": r3_cases, "R4": r4_cases}
LARGE = ("S7", "W3")  # plain bytes of 8 MiB: pyoracle (a byte loop in Python) runs one case of each
