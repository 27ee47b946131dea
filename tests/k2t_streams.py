"""The stream groups of the K2t suite (ez_decompress_tok.hip; tests/test_gpu_k2t.py).

K2t stages the input in scan windows of 1,024 positions: a window starts at base = w & ~15, where
w is the first token start at or after the previous base + 1024 (w = 0 first).  A window's tokens
go through rounds of up to 64 tokens, one per lane; a round ends early before a token longer than
kTBig = 512 bytes (moved alone) and before the token whose running output passes the budget
(R - 1024 - 64: 3,008 with the 4 KiB ring, 7,104 with the 8 KiB one).  Copies of a round read the
ring from ringlo = pos + total - R + 16 on and HBM below, and run in batches that end before the
first copy whose source reaches past the batch's first output byte (need > oa).

S (below) builds a stream token by token and keeps the input offset, the output position and the
token starts, so that a group can place a token at a given offset of its window and a copy at a
given source."""

import numpy as np

from k2_streams import HDR, META_BREAK, META_RESET, _forms, cpy, cpy_long, lit, meta, rb

BUDGETS = (3008, 7104)  # TLayout<4096>::budget, TLayout<8192>::budget
T_WIN = 1024
T_BIG = 512


class S:
    """A stream under construction: c its bytes, pos the output position, starts the token starts
    (every padding zero is a token of its own for K2t's scan)."""

    def __init__(self, rng, c=HDR):
        self.rng, self.c, self.pos, self.starts = rng, b"", 0, []
        if c:
            self.raw(c[:6], 0)
            self.raw(c[6:], 0)

    def raw(self, tok, out_len):
        if tok:
            self.starts.append(len(self.c))
            self.c += tok
            self.pos += out_len
        return self

    def lit(self, n=None, body=None):
        body = rb(self.rng, n) if body is None else body
        return self.raw(lit(body), len(body))

    def cpy(self, d, n, long=False):
        return self.raw((cpy_long if long else cpy)(d, n), n)

    def src(self, at, n, long=False):
        """A copy of n bytes whose source starts at output position `at`."""
        return self.cpy(self.pos - at, n, long)

    def zeros(self, n):
        for _ in range(n):
            self.raw(b"\x00", 0)
        return self

    def brk(self):
        return self.raw(meta(META_BREAK), 0)

    def window(self):
        """(base, end) of the scan window that holds the next token's start."""
        pts = self.starts + [len(self.c)]
        w = 0
        while True:
            base = w & ~15
            nxt = [p for p in pts if p >= base + T_WIN]
            if not nxt:
                return base, base + T_WIN
            w = nxt[0]

    def to(self, target):
        """Literals up to input offset `target` (as k2_streams.lit_to: up to three 1-byte literals and
        one that ends there)."""
        for extra in range(4):
            for tl in (1, 2, 3, 5):
                n = target - len(self.c) - 2 * extra - tl
                if n >= 1 and len(lit(bytes(n))) == tl + n:
                    for _ in range(extra):
                        self.lit(1)
                    self.lit(n)
                    assert len(self.c) == target
                    return self
        raise AssertionError((len(self.c), target))

    def new_window(self):
        """Literals up to the end of the current window: the next token opens a window."""
        base, end = self.window()
        return self.to(end if end >= len(self.c) + 2 else end + T_WIN)

    def trailer(self):
        return self.lit(4).cpy(3, 12)

    def done(self):
        return self.c


def stamped(rng, n):
    """n bytes of 40-byte records, each a 4-byte counter and random bytes: a source off by any
    amount shows."""
    out = b""
    k = 0
    while len(out) < n:
        out += k.to_bytes(4, "little") + rb(rng, 36)
        k += 1
    return out[:n]


def filler20(rng):
    """A valid stream of 20 bytes (the batches of 3,300 streams that take the 4 KiB ring)."""
    s = HDR + lit(rb(rng, 8)) + cpy(5, 5)
    assert len(s) == 20
    return s


# ---------------------------------------------------------------- T1: scan seams

RARE = ("lit_len1", "lit_len2", "lit_len4", "cpy_len1_off1", "cpy_len2", "cpy_off4", "cpy_len4_run", "cpy_long", "zero_region", "break", "ver", "magic")


def _first(rng, far):
    s = S(rng)
    if far:
        s.lit(70000)
    return s


def t1_streams():
    """Every form of _forms with its header starting k = 0 .. header length bytes before the end of a
    scan window: the first window's (offset 1024) and a later, drifted one (a literal straddles the
    first window's end, so the second window starts at an offset that is no multiple of 1024); every
    form starting at every offset mod 16 (the rare forms at a lane segment's first and last position
    among them); two rare forms back to back; the 70,000-byte literal as a window's last token
    (k = 1..5 of lit_len4: an advance over 65,535, the exits' 0xffff clamp)."""
    rng = np.random.default_rng(2101)
    out = []
    forms = _forms(rng)
    for name, form, hlen, far in forms:
        outl = {"lit_len0": 50, "lit_len1": 200, "lit_len2": 1000, "lit_len4": 70000, "cpy_len1_off1": 200, "cpy_len2": 500,
                "cpy_len4_run": 70000, "zero_region": 64}.get(name, 20 if name.startswith("cpy") else 0)
        for k in range(hlen + 1):
            s = _first(rng, far).lit(600)
            base, end = s.window()
            s.to(end - k).raw(form, outl).trailer()
            if not far:
                assert end == 1024
            out.append((f"t1-{name}-first-k{k}", s.done()))
            s = _first(rng, far).lit(600)
            base, end = s.window()
            s.to(end - 24).lit(200)  # straddles the window's end: the next window starts past it
            base2, end2 = s.window()
            assert base2 > end and end2 % 1024 != 0 and base2 % 16 == 0
            s.to(end2 - k).raw(form, outl).trailer()
            out.append((f"t1-{name}-drift-k{k}", s.done()))
        for r in range(16):
            s = _first(rng, far).lit(600)
            at = (len(s.c) + 40) // 16 * 16 + 16 + r
            s.to(at).raw(form, outl).trailer()
            out.append((f"t1-{name}-mod16_{r}", s.done()))
    # a literal that advances 65,536 + 20 bytes from the middle of a window (its last token all the
    # same): an exit stored as its low 16 bits instead of clamped would point 20 bytes past the
    # header, inside the window, and mark token starts in the literal's body (which holds a
    # 123-byte literal tag there and every 124 bytes on, so such a walk stays on plain forms)
    for at in (500, 511, 512):
        body = bytearray(rb(rng, 65553))
        body[17::124] = b"\x7b" * len(body[17::124])
        s = S(rng).lit(300)
        s.to(at).lit(body=bytes(body))
        assert len(lit(bytes(body))) == 65536 + 20 and s.window()[0] > 65536
        out.append((f"t1-lit-advance-65556-at{at}", s.trailer().done()))
    by = {name: (form, hlen, far) for name, form, hlen, far in forms}
    for a in RARE:
        for b in RARE:
            if by[a][2] or by[b][2] or "len4" in a or "len4" in b:
                continue
            s = S(rng).lit(700)
            s.c += by[a][0] + by[b][0]  # (checked against the oracle only: S's bookkeeping ends here)
            out.append((f"t1-{a}+{b}", s.c + lit(rb(rng, 4)) + cpy(3, 12)))
    return out


# ---------------------------------------------------------------- T2: rounds


def t2_streams():
    """Windows of exactly 63, 64, 65, 128 and 512 tokens (1-byte literals), a window of 1,024 padding
    zeros, Breaks inside a round, 100 padding zeros before the header (the MetaReset is parsed in the
    second round, at pos 0), magic + padding + reset (the reset on another lane than 0)."""
    rng = np.random.default_rng(2102)
    out = []
    for n in (63, 64, 65, 128, 512):
        s = S(rng).lit(500).new_window()
        base, end = s.window()
        assert base == len(s.c) == 1024
        for _ in range(n - 1):
            s.lit(1)
        if n < 512:
            s.lit(end - len(s.c) + 50)  # the window's last token, ending past it
        else:
            s.lit(1)
            assert len(s.c) == end
        assert sum(base <= p < end for p in s.starts) == n
        out.append((f"t2-window-{n}-tokens", s.trailer().done()))
    s = S(rng).lit(500).new_window().zeros(1024)
    assert len(s.c) == 2048
    out.append(("t2-window-of-zeros", s.lit(30).cpy(17, 40).trailer().done()))
    s = S(rng).lit(300)
    for k in range(40):
        s.lit(3).cpy(100 + k, 7)
        if k % 3 == 0:
            s.brk()
    out.append(("t2-breaks", s.trailer().done()))
    s = S(rng, c=b"").zeros(100)
    s.raw(HDR[:6], 0).raw(HDR[6:], 0)
    out.append(("t2-100-zeros-before-header", s.lit(50).cpy(20, 30).trailer().done()))
    s = S(rng, c=b"").raw(HDR[:6], 0).zeros(5).raw(HDR[6:], 0)
    out.append(("t2-magic-padding-reset", s.lit(50).cpy(20, 30).trailer().done()))
    return out


def t2_two_resets():
    """Two MetaResets before any output (which decoder takes it is not prescribed)."""
    rng = np.random.default_rng(2103)
    return [("t2-two-resets", S(rng).raw(meta(META_RESET, b"\x12"), 0).lit(50).cpy(20, 30).trailer().done())]


# ---------------------------------------------------------------- T3: budget and kTBig


def t3_streams():
    """Single tokens of 511, 512 and 513 bytes (a literal, a copy, a run: 513 is moved alone); rounds
    whose running output reaches budget - 1, budget and budget + 1 at lane 7 or 8 (both budgets); a
    512-byte token that ends exactly on the budget."""
    rng = np.random.default_rng(2104)
    out = []
    for L in (T_BIG - 1, T_BIG, T_BIG + 1):
        out.append((f"t3-lit-{L}", S(rng).lit(100).lit(L).trailer().done()))
        out.append((f"t3-cpy-{L}", S(rng).lit(700).cpy(600, L).trailer().done()))
        out.append((f"t3-cpy-overlap-{L}", S(rng).lit(700).cpy(40, L).trailer().done()))
        out.append((f"t3-run-{L}", S(rng).lit(100).cpy(3, L).trailer().done()))
    for budget in BUDGETS:
        n512 = (budget - 448) // 512
        assert budget == 448 + 512 * n512
        for delta in (-1, 0, 1):
            s = S(rng).lit(650).new_window()
            p0 = s.pos
            for k in range(n512):
                s.cpy(520 + 13 * k, 512)
            s.lit(100).cpy(555, 348 + delta)
            assert s.pos - p0 == budget + delta
            for k in range(10):
                s.lit(2).cpy(700 + k, 30)
            out.append((f"t3-budget-{budget}{delta:+d}", s.trailer().done()))
        s = S(rng).lit(650).new_window()
        p0 = s.pos
        s.lit(100).cpy(555, 348)
        for k in range(n512):
            s.cpy(520 + 13 * k, 512)
        assert s.pos - p0 == budget
        out.append((f"t3-512-lands-on-budget-{budget}", s.lit(5).cpy(530, 512).trailer().done()))
    return out


# ---------------------------------------------------------------- T4: ring reach


def t4_streams(R):
    """Copies of 200 bytes with every D in [R - 1104, R + 48], each the first, a middle or the last
    token of a round that fills its budget exactly (so the next token starts a round): its source
    lies on both sides of ringlo = pos + total - R + 16 and straddles it.  The output before the
    rounds is stamped with a counter every 40 bytes.  12 rounds a stream, all in one scan window."""
    rng = np.random.default_rng(2105 + R)
    budget = R - 1024 - 64
    n512, rem = (budget - 200) // 512, (budget - 200) % 512
    assert rem > 0
    probes = [(D, where) for D in range(R - 1104, R + 49) for where in (0, 1, 2)]
    out = []
    for g in range(0, len(probes), 12):
        s = S(rng).lit(body=stamped(rng, R + 1200)).new_window()
        base, end = s.window()
        for D, where in probes[g : g + 12]:
            p0 = s.pos
            fill = [int(rng.integers(600, 1100)) for _ in range(n512)]
            at = (0, n512 // 2, n512)[where]
            for k in range(n512 + 1):
                if k == at and where < 2:
                    s.cpy(D, 200)
                if k < n512:
                    s.cpy(fill[k], 512)
            s.cpy(int(rng.integers(600, 1100)), rem)
            if where == 2:
                s.cpy(D, 200)
            assert s.pos - p0 == budget
        assert len(s.c) < end - 16  # (every round's tokens in the one window)
        out.append((f"t4-R{R}-D{probes[g][0]}..", s.trailer().done()))
    return out


# ---------------------------------------------------------------- T5: copy batches


def t5_streams():
    """Copies whose source ends exactly at an earlier copy's first output byte and one byte past it
    (the batch rule need > oa); D in 15, 16, 17 with L > D; 64 copies in one round, each reading the
    one before; rounds with >= 16 copies that read the round's own output: sources inside an earlier
    copy (the redirect, once and twice deep), inside a literal, straddling two tokens, with zero-length
    tokens (padding, a Break) between tokens that share an output position."""
    rng = np.random.default_rng(2106)
    out = []
    for past in (0, 1, 2, 15, 16, 17):
        for L in (5, 16, 20, 33):
            s = S(rng).lit(700).new_window()
            oa = s.pos
            s.cpy(600, 40).lit(30)
            s.src(oa - L + past, L)  # its source ends `past` bytes into the first copy's output
            out.append((f"t5-source-ends-{past}-past-L{L}", s.lit(3).cpy(50, 20).trailer().done()))
    for D in (15, 16, 17):
        for L in (D + 1, 40, 300):
            out.append((f"t5-D{D}-L{L}", S(rng).lit(700).new_window().cpy(600, 30).cpy(D, L).lit(2).cpy(D, L).trailer().done()))
    for L in (1, 16, 20):
        s = S(rng).lit(700).new_window().lit(L)
        for _ in range(64):
            s.cpy(L, L)
        out.append((f"t5-chain-64-L{L}", s.trailer().done()))
    s = S(rng).lit(700).new_window().lit(24)
    for k in range(64):
        s.cpy(24 + (k % 3), 20 + (k % 5))
    out.append(("t5-chain-64-mixed", s.trailer().done()))
    for gap in ("", "pad", "brk"):
        s = S(rng).lit(700).new_window()
        for k in range(7):
            a = s.pos
            s.lit(40)  # [a, a + 40)
            if gap == "pad":
                s.zeros(1 + k % 3)
            if gap == "brk":
                s.brk()
            b = s.pos
            s.src(a + 5, 20)  # inside the literal: [b, b + 20)
            c = s.pos
            s.src(b + 2, 16)  # inside the copy before it (one redirect, into the literal)
            d = s.pos
            s.src(c, 16)  # inside that one (two redirects)
            s.src(a + 30, 20)  # straddles the literal and the first copy
            s.src(d - 8, 24)  # straddles two copies
            if gap == "pad":
                s.zeros(2)
            s.src(b + 1, 19, long=True)  # the long prefix, inside a copy
        out.append((f"t5-own-output-{gap or 'plain'}", s.trailer().done()))
    return out


# ---------------------------------------------------------------- T6: tokens moved alone, deferred literals

DEFER_MIN = 16384  # kDeferMin


def t6_streams():
    """Literals of 16,383, 16,384 and 16,385 bytes (kDeferMin = 16,384); nine literals of 16,384
    bytes or more in one stream (kDefSlots = 8: the ninth is moved at once); after a deferred
    literal: copies and runs reading across its first and its last byte, a 600-byte copy with D in
    16, 17, 1023, 1024, 1025, a 600-byte run; D > pos on the round path and on the alone path."""
    rng = np.random.default_rng(2107)
    out = []
    for n in (DEFER_MIN - 1, DEFER_MIN, DEFER_MIN + 1):
        s = S(rng).lit(100).lit(n)
        out.append((f"t6-lit-{n}", s.cpy(n + 50, 30).cpy(20, 600).trailer().done()))
    s = S(rng).lit(100)
    for k in range(9):
        s.lit(DEFER_MIN + k).cpy(DEFER_MIN + k + 10, 40).cpy(DEFER_MIN // 2, 700)
    out.append(("t6-nine-long-literals", s.cpy(9 * DEFER_MIN, 900).trailer().done()))
    for tail in ("round", "alone"):
        L = 40 if tail == "round" else 600
        s = S(rng).lit(100)
        a = s.pos
        s.lit(DEFER_MIN + 7)
        b = s.pos
        s.src(a - 10, L).src(b - 10, L).src(a - 3, L + 1).src(b - L - 5, L).src(b - 1, L)
        s.lit(3).cpy(3, L).src(a, L).src(a - 1, L)
        out.append((f"t6-across-deferred-{tail}", s.trailer().done()))
    for D in (16, 17, 1023, 1024, 1025):
        out.append((f"t6-after-deferred-cpy600-D{D}", S(rng).lit(100).lit(DEFER_MIN + 3).cpy(D, 600).lit(2).cpy(D, 600).trailer().done()))
    for D in (1, 3, 15):
        out.append((f"t6-after-deferred-run600-D{D}", S(rng).lit(100).lit(DEFER_MIN + 3).cpy(D, 600).lit(2).cpy(D, 600).trailer().done()))
    for L in (40, 600):
        for D in (16, 100, 5000):
            out.append((f"t6-before-start-D{D}-L{L}", S(rng).lit(9).cpy(D, L).lit(3).cpy(D + L + 20, L).trailer().done()))
            out.append((f"t6-before-start-first-D{D}-L{L}", S(rng).cpy(D, L).lit(3).trailer().done()))
    return out


# ---------------------------------------------------------------- T7: slots


def t7_streams():
    """(name, stream, output bytes up to and including the token under test): the slot is sized to
    exactly that and to one byte less, at a token on the round path and at a token moved alone."""
    rng = np.random.default_rng(2108)
    out = []
    for nm, L in (("round", 40), ("round-512", 512), ("alone", 513), ("alone-lit", 2000)):
        for kind in ("cpy", "lit"):
            s = S(rng).lit(700).lit(5).cpy(100, 30)
            if kind == "cpy":
                s.cpy(600, L)
            else:
                s.lit(L)
            out.append((f"t7-{nm}-{kind}", s.done(), s.pos))
    return out
