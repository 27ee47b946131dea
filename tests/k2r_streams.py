"""The stream groups of the K2r suite (ez_decompress_ring.hip), shared by its GPU half
(tests/test_gpu_k2r.py) and its CPU half (tests/test_ring_emu.py through tools/ring_emu).

Each group is a list of Case(name, stream, slot): slot None takes the default slot (the oracle's
length plus 1..5 bytes).  Literals are random bytes, so no content has a period that divides a
distance under test; a tail (a short literal and a copy of it plus older bytes) follows every probe
so that a ring left wrong by the probe shows in later bytes too.

The constants the groups sit on (ez_decompress_ring.hip): kRing = 512, kNear = kRing - 16 = 496
(copies up to this distance read the ring, farther ones HBM), the pair rule o2 = 1 + L1 <= 11 and
16 - o2 - adv2 >= 0 (a short literal and the copy after it in one step), the flush bound (at most
kChunk + 31 * 9 + 16 <= kRing unflushed bytes) and ring_st's mirror and guard writes."""

from collections import namedtuple

import numpy as np

from k2_streams import HDR, HDR_1K, META_RESET, _need, _oracle, cpy, cpy_long, lit, meta, rb

Case = namedtuple("Case", "name stream slot")
Case.__new__.__defaults__ = (None,)

def tail(rng):
    return lit(rb(rng, 5)) + cpy(20, 18) + lit(rb(rng, 2))


def lag_builder(rng, steps=9):
    """`steps` pair steps, a 10-byte literal and a 16-byte near copy each (26 bytes of output in one
    step, the most a step moves): the output not yet flushed grows as fast as the kernel allows."""
    out = b""
    for _ in range(steps):
        out += lit(rb(rng, 10)) + cpy(int(rng.integers(40, 400)), 16)
    return out


# ---------------------------------------------------------------- R1: the ring / HBM threshold

R1_D = range(481, 529)
R1_L = (1, 15, 16, 17, 33, 123, 124, 300)


def r1_streams():
    """Probe copies with D in 481..528 (kNear = 496 in the middle) and every L, after a lag builder of
    9..16 pair steps (so the far copy's HBM source is loaded with as much output unflushed as can
    be), after a short-period run, and after a plain 100-byte literal."""
    rng = np.random.default_rng(1101)
    out = []
    for D in R1_D:
        for L in R1_L:
            steps = 9 + (D + L) % 8  # (the probe at every phase of the flush period of 8 steps)
            for ctx, before in (("lag", lag_builder(rng, steps)), ("run", lit(rb(rng, 3)) + cpy(3, 61)), ("lit", lit(rb(rng, 100)))):
                first = 530 + int(rng.integers(0, 128))
                out.append(Case(f"r1-{ctx}-D{D}-L{L}", HDR + lit(rb(rng, first)) + before + cpy(D, L) + tail(rng)))
    return out


# ---------------------------------------------------------------- R2: ring residues


def r2_streams():
    """A literal of p bytes for every p in 0..527, then a near copy, a far copy, a run or a
    15-byte literal: ring_st starts at every residue (r < 16 writes the mirror, r + 16 > 512 wraps
    into the front guard).  p < D reads the zero history before the stream start."""
    rng = np.random.default_rng(1102)
    out = []
    for p in range(528):
        pre = HDR + (lit(rb(rng, p)) if p else b"")
        out.append(Case(f"r2-p{p}-near", pre + cpy(100, 40) + tail(rng)))
        out.append(Case(f"r2-p{p}-far", pre + cpy(497, 40) + tail(rng)))
        out.append(Case(f"r2-p{p}-run", pre + cpy(3, 40) + tail(rng)))
        out.append(Case(f"r2-p{p}-lit", pre + lit(rb(rng, 15)) + tail(rng)))
    return out


# ---------------------------------------------------------------- R3: runs and zero regions

R3_L = tuple(range(1, 49)) + (123, 124, 379, 380, 1000)


def r3_streams():
    """Runs (D in 1..15) and zero regions (D = 0) of every L at output phases 5, 500 and 509 mod
    512; runs whose distance reaches before the stream start, a run as the first token, a run right
    after a pair, and a run right after a 1-byte literal (the pattern's source is stored in the
    same step)."""
    rng = np.random.default_rng(1103)
    out = []
    for ph in (5, 500, 509):
        for D in range(16):
            for L in R3_L:
                out.append(Case(f"r3-ph{ph}-D{D}-L{L}", HDR + lit(rb(rng, ph)) + cpy(D, L) + tail(rng)))
    for D in range(1, 16):
        for L in (1, 16, 40):
            if D >= 2:  # (D = 1 before the start: the run as the first token, below)
                out.append(Case(f"r3-before-start-D{D}-L{L}", HDR + lit(rb(rng, D // 2)) + cpy(D, L) + tail(rng)))
            out.append(Case(f"r3-first-D{D}-L{L}", HDR + cpy(D, L) + tail(rng)))
            out.append(Case(f"r3-after-pair-D{D}-L{L}", HDR + lit(rb(rng, 300)) + lit(rb(rng, 7)) + cpy(120, 16) + cpy(D, L) + tail(rng)))
            out.append(Case(f"r3-after-lit1-D{D}-L{L}", HDR + lit(rb(rng, 200)) + lit(rb(rng, 1)) + cpy(D, L) + tail(rng)))
    return out


# ---------------------------------------------------------------- R4: literal + copy pairs

R4_LIMIT = 8  # BlockSizeLimit of r4_limit_streams (their window is 8 bytes too)


def _r4_copies():
    """(name, copy token, bytes of output needed before the pair, header) -- every header form
    (plain 2 bytes, long prefix 3, Off1 3, Off1 + prefix 4, Off2 4, Off2 + prefix 5) with the
    copy kinds it can express."""
    c = []
    for nm, tok in (("plain", cpy(100, 20)), ("long", cpy_long(100, 20)), ("off1", cpy(320, 20)), ("off1-long", cpy_long(320, 20))):
        c.append((f"near-{nm}", tok, 400, HDR))
    c.append(("near-plain-496", cpy(496, 123), 600, HDR))
    c.append(("near-off1-496", cpy(496, 20), 600, HDR))
    for D in range(497, 513):
        c.append((f"far-D{D}-off1", cpy(D, 20), 700, HDR))
        c.append((f"far-D{D}-{'off1' if D < 508 else 'off2'}-long", cpy_long(D, 20), 700, HDR))
    c.append(("far-off2", cpy(800, 20), 900, HDR))
    c.append(("far-off2-long", cpy_long(800, 20), 900, HDR))
    for D in range(1, 16):
        c.append((f"run-D{D}-plain", cpy(D, D), 300, HDR))  # (L2 = D: offset byte 0)
        c.append((f"run-D{D}-long", cpy(D, 40), 300, HDR))  # (L2 > D: the long prefix)
    c.append(("zero", cpy(0, 20), 300, HDR))
    for D in (1024, 1025):  # the window and one more, under a 1 KiB reset (1025: an error, handed over)
        c.append((f"window-D{D}-off2", cpy(D, 20), 1100, HDR_1K))
        c.append((f"window-D{D}-off2-long", cpy_long(D, 20), 1100, HDR_1K))
    return c


def r4_streams():
    """Every L1 in 1..15 before every copy form and kind (o2 = 1 + L1 on both sides of 11, and of
    16 - o2 - adv2 >= 0 for header lengths 2..5); the pair mid-stream and as the stream's last two
    tokens; a pair whose copy overflows its slot by exactly one byte (ENOSPC, handed over)."""
    rng = np.random.default_rng(1104)
    out = []
    for L1 in range(1, 16):
        for nm, tok, first, hdr in _r4_copies():
            s = hdr + lit(rb(rng, first)) + lit(rb(rng, L1)) + tok
            out.append(Case(f"r4-L1_{L1}-{nm}", s + tail(rng)))
            if nm in ("near-plain", "near-off1-long", "far-D500-off1", "far-D510-off2-long", "run-D3-long", "run-D7-plain", "zero"):
                out.append(Case(f"r4-L1_{L1}-{nm}-last", s))
                need = _need(s)
                if need - 1 >= 16:
                    out.append(Case(f"r4-L1_{L1}-{nm}-slot-1", s, need - 1))
                out.append(Case(f"r4-L1_{L1}-{nm}-slot-exact", s, need))
    return out


def r4_limit_streams():
    """BlockSizeLimit = 8 (with an 8-byte window, the largest the limit admits): L1 and L2 equal to
    the limit and one more (EBLOCKLIMIT, handed over), in pairs of every header form that 8 bytes
    of distance can express."""
    rng = np.random.default_rng(1105)
    hdr = b"\x80\x02eazy" + meta(META_RESET, b"\x03")
    out = []
    for L1 in (1, 7, 8, 9, 10):
        for L2, D in ((8, 8), (9, 8), (8, 3), (9, 3), (8, 0), (9, 0), (3, 8), (3, 9)):
            for form in (cpy, cpy_long):
                s = hdr + lit(rb(rng, 8)) + cpy(8, 8) + lit(rb(rng, L1)) + form(D, L2) + lit(rb(rng, 3))
                out.append(Case(f"r4-limit-L1_{L1}-L2_{L2}-D{D}-{form.__name__}", s))
    return out


# ---------------------------------------------------------------- R5: batch and slot edges


def r5_last_stream_batches():
    """Batches [a neighbour, the stream under test last]: the last stream's final loads are clamped
    to the batch's last 16 bytes.  Tails: a literal of 1..20 bytes, a copy header, literals of 17,
    31, 32 and 33 bytes (the long-literal path); a last stream shorter than 16 bytes in all."""
    rng = np.random.default_rng(1106)
    first = HDR + lit(rb(rng, 300)) + cpy(200, 100)
    batches = []
    body = HDR + lit(rb(rng, 40)) + cpy(30, 25)
    for n in list(range(1, 21)) + [31, 32, 33]:
        batches.append((f"r5-last-lit{n}", [Case("first", first), Case("last", body + lit(rb(rng, n)))]))
    for nm, tok in (("plain", cpy(30, 20)), ("off1", cpy(300, 20)), ("off2-long", cpy_long(600, 20)), ("run", cpy(1, 90))):
        batches.append((f"r5-last-cpy-{nm}", [Case("first", first), Case("last", body + tok)]))
    for nm, s in (("hdr-only", HDR), ("hdr-lit3", HDR + lit(b"xyz")), ("hdr-run", HDR + cpy(0, 5)), ("empty", b""), ("magic-only", HDR[:6])):
        batches.append((f"r5-last-short-{nm}", [Case("first", first), Case("last", s)]))
    return batches


def r5_tiny_batches():
    """Batches of less than 16 input bytes in all: K2r hands every stream over (its clamped loads
    need 16 bytes), and the results are still the oracle's."""
    return [
        ("r5-tiny-one", [Case("a", HDR + lit(b"abc"))]),
        ("r5-tiny-two", [Case("a", HDR[:6]), Case("b", HDR)]),
        ("r5-tiny-empty", [Case("a", b""), Case("b", b""), Case("c", HDR + lit(b"q"))]),
    ]


def r5_streams():
    """A first stream whose first token is a far copy from before the stream start (zeros, not the
    bytes before its slot); empty and header-only streams between others; slots of exactly the needed
    size; slots of 15, 16 and 17 bytes (under 16: handed over)."""
    rng = np.random.default_rng(1107)
    out = [Case("r5-first-far-copy", HDR + cpy(600, 50) + lit(rb(rng, 30)) + cpy(60, 70) + tail(rng))]
    good = [HDR + lit(rb(rng, 600)) + cpy(497, 60) + lit(rb(rng, 9)) + cpy(100, 16) + cpy(2, 33) + tail(rng) for _ in range(4)]
    out += [Case("r5-empty", b""), Case("r5-good0", good[0]), Case("r5-hdr-only", HDR), Case("r5-empty2", b""), Case("r5-magic-only", HDR[:6])]
    for k, g in enumerate(good):
        out.append(Case(f"r5-exact-slot-{k}", g, _need(g)))
    for n in (10, 14, 15, 16, 17, 18):
        s = HDR + lit(rb(rng, 5)) + cpy(3, n - 5)
        for slot in (15, 16, 17):
            out.append(Case(f"r5-need{n}-slot{slot}", s, slot))
    out.append(Case("r5-empty-last", b""))
    return out


# ---------------------------------------------------------------- R6: a mixed wave


def _big(rng):
    """40 KiB of output from ~100 bytes of input: a literal, then long runs and copies."""
    s = HDR + lit(rb(rng, 700))
    for k in range(20):
        s += cpy((1, 7, 15, 0, 600, 497)[k % 6], 1000 + 37 * k) + lit(rb(rng, 3)) + cpy(int(rng.integers(16, 690)), 700 - k)
    assert 35000 < _need(s) < 48000
    return s


def r6_streams():
    """327 streams (a block of 256, a wave of 64 and 7): neighbouring lanes hold an empty stream, a
    1-byte output, a 40 KiB output, ordinary streams, truncated and bit-flipped ones and a slot too
    small."""
    rng = np.random.default_rng(1108)
    out = []
    for s in range(327):
        g = HDR + lit(rb(rng, 120)) + lag_builder(rng, 6) + lit(rb(rng, 500)) + cpy(int(rng.integers(480, 530)), 90) + cpy(int(rng.integers(0, 16)), 50) + tail(rng)
        k = s % 9
        if k == 0:
            out.append(Case(f"r6-{s}-empty", b""))
        elif k == 1:
            out.append(Case(f"r6-{s}-one-byte", HDR + lit(b"Z")))
        elif k == 2 and s % 27 == 2:
            out.append(Case(f"r6-{s}-big", _big(rng)))
        elif k == 3:
            out.append(Case(f"r6-{s}-truncated", g[: int(rng.integers(10, len(g)))]))
        elif k == 4:
            x = bytearray(g)
            x[int(rng.integers(0, len(g)))] ^= 1 << int(rng.integers(0, 8))
            out.append(Case(f"r6-{s}-bit-flip", bytes(x)))
        elif k == 5:
            out.append(Case(f"r6-{s}-small-slot", g, _need(g) - int(rng.integers(1, 200))))
        else:
            out.append(Case(f"r6-{s}-good", g))
    return out


def expected_handed(cases, limit=0):
    """The indices the decoder must hand over: the streams the oracle gives an error for, or whose
    output does not fit the slot."""
    bad = set()
    for s, c in enumerate(cases):
        if c.slot is not None and c.slot < 16:
            bad.add(s)  # (K2r's and K2t's clamped 16-byte accesses need a slot of 16 bytes)
        elif c.slot is not None:
            if _oracle(c.stream, c.slot, limit)[1] != 0:
                bad.add(s)
        elif _oracle(c.stream, max(1 << 20, 4 * len(c.stream)), limit)[1] != 0:
            bad.add(s)
    return bad
