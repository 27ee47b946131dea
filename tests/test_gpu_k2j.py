"""K2j (eazy_amd/csrc/ez_decompress_jump.hip) on hand-built streams, against the oracle.

K2j guesses token starts per chunk of the compressed stream (256 bytes for a batch of at most 96 KiB
of input, 1 KiB above), repairs wrong guesses in order (kj_fix) and resolves copies by pointer
jumping.  The log streams of the other tests barely exercise the repairs: a wrong start meets the
true chain within ~110 bytes.  The streams here are built token by token (ez.Encoder) so that token
headers straddle chunk seams at every byte position, speculation never meets the true chain,
literal bodies look like tokens, copy chains are tens of thousands deep, and batches have the
shapes at which the per-stream and per-chunk loops change path.

Every decode forces K2j, and checks, per stream: status, size and bytes equal the oracle's
(orc.decompress with the slot as capacity) and the exact decoder's; every output byte outside
[out_off[s], out_off[s] + size) keeps its 0xA5 sentinel (slot slack and the bytes before out_off[0]
included); and the streams K2j handed to the exact decoder (the workspace's first words: the count,
then the stream indices) are exactly the ones expected -- none, for valid streams of the forms K2j
takes.  All comparisons are exact equality.  The builders and the check (_run) live in
tests/k2_streams.py, shared with the K2r and K2t suites."""

import numpy as np
import pytest

import oracle as orc
from k2_streams import HDR, META_RESET, SMALL_MAX, _forms, _need, _oracle, _run, cpy, lit, lit_to, meta, rb

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the streams (builders: k2_streams)


def _trailer():
    return lit(b"tail") + cpy(3, 12)


def seam_streams():
    """Each form once per header position: the header starts k bytes before a seam (a multiple of
    1 KiB: a seam at both chunk sizes) for k = 0 .. its length; a preceding literal aligns it."""
    rng = np.random.default_rng(101)
    out = []
    for name, form, hlen, far in _forms(rng):
        assert len(form) >= hlen
        for k in range(hlen + 1):
            c = HDR + (lit(rb(rng, 70000)) if far else b"")
            seam = (len(c) + 1100) // 1024 * 1024
            c = lit_to(c, seam - k, rng)
            out.append((f"{name}-k{k}", c + form + _trailer()))
    # a token that ends exactly on a seam which is the stream's last byte (a copy, a literal)
    c = lit_to(HDR, 1024 - 2, rng) + cpy(30, 20)
    assert len(c) == 1024
    out.append(("copy-ends-stream-on-seam", c))
    c = lit_to(lit_to(HDR, 1000, rng) + cpy(7, 40), 2048, rng)
    assert len(c) == 2048
    out.append(("literal-ends-stream-on-seam", c))
    # ... and one whose last token ends one byte past / before a seam
    out.append(("ends-seam+1", lit_to(HDR, 1025 - 2, rng) + cpy(30, 20)))
    out.append(("ends-seam-1", lit_to(HDR, 1023 - 2, rng) + cpy(30, 20)))
    return out


def phase_stream(first, nbytes):
    """The header, a literal of `first` bytes, then `86 05` (copy, L = 6, D = 11) repeated up to
    nbytes of input.  Read from the wrong parity every 0x05 is a 5-byte literal, so a walk that
    starts off phase never meets the true chain."""
    c = HDR + lit(bytes(range(65, 65 + first)))
    start = len(c)
    c += cpy(11, 6) * ((nbytes - start) // 2)
    assert cpy(11, 6) == b"\x86\x05"
    return c, start


def body_streams():
    """Literals of 3,000 and 70,000 bytes whose bodies look like tokens, then short copies into them."""
    rng = np.random.default_rng(103)
    out = []
    for n in (3000, 70000):
        fills = [("00", bytes(n)), ("8080", b"\x80" * n), ("7e", b"\x7e" * n), ("ff", b"\xff" * n), ("fc", b"\xfc" * n),
                 ("fd", b"\xfd" * n), ("fe", b"\xfe" * n), ("random", rb(rng, n))]
        for name, body in fills:
            out.append((f"body-{name}-{n}", HDR + lit(body) + cpy(100, 20) + cpy(n - 1, 50) + cpy(1, 30) + lit(b"z") + cpy(n // 2, 300)))
    return out


def copy_streams():
    rng = np.random.default_rng(105)
    out = [
        ("run-of-a", HDR + lit(b"a") + cpy(1, 65915) * 3),
        ("period-7", HDR + lit(rb(rng, 7)) + cpy(7, 5000) + lit(b"x") + cpy(8, 100)),
    ]
    small = b"\x80\x02eazy" + meta(META_RESET, b"\x0a")  # a 1 KiB window
    out.append(("distance-window", small + lit(rb(rng, 1100)) + cpy(1024, 10) + lit(b"y")))
    out.append(("distance-window+1", small + lit(rb(rng, 1100)) + cpy(1025, 10) + lit(b"y")))
    return out


_FILLER = None


def filler():
    """A valid stream of more than 96 KiB of input: with it a batch takes 1 KiB chunks."""
    global _FILLER
    if _FILLER is None:
        rng = np.random.default_rng(107)
        _FILLER = HDR + lit(rb(rng, 100000)) + cpy(500, 60) + lit(b"end") + cpy(99000, 1000)
        assert len(_FILLER) > SMALL_MAX
    return _FILLER


# ---------------------------------------------------------------- the check (k2_streams._run)


def _both(cuda, ins, handed="auto", slots=None, hints=None, filler_at=None):
    """Every group at both chunk sizes: the streams in batches of at most 96 KiB of input (256-byte
    chunks), then all of them and a filler stream (checked too) that lifts the input over it."""
    idx, size = [], 0
    batches = []
    for s, b in enumerate(ins):
        if len(b) > SMALL_MAX:
            continue  # (such a stream takes 1 KiB chunks alone)
        if idx and size + len(b) > SMALL_MAX:
            batches.append(idx)
            idx, size = [], 0
        idx.append(s)
        size += len(b)
    if idx:
        batches.append(idx)
    for idx in batches:
        sub_slots = {k: slots[s] for k, s in enumerate(idx) if slots and s in slots}
        sub_handed = handed if handed in ("auto", "all", None) else {k for k, s in enumerate(idx) if s in handed}
        _run(cuda, [ins[s] for s in idx], 256, slots=sub_slots, handed=sub_handed, hints=hints)
    m = len(ins) // 2 if filler_at is None else filler_at
    shift = lambda s: s if s < m else s + 1  # noqa: E731
    _run(cuda, ins[:m] + [filler()] + ins[m:], 1024, slots={shift(s): v for s, v in (slots or {}).items()},
         handed=handed if handed in ("auto", "all", None) else {shift(s) for s in handed}, hints=hints)


# ---------------------------------------------------------------- the groups


def test_k2j_seams(cuda):
    """Token headers straddling a chunk seam at every byte position: literals with Len0 / Len1 /
    Len2 / Len4 lengths, copies with plain / Off1 / Off2 / Off4 offsets and Len1 / Len2 / Len4
    lengths, the long prefix, a zero region, Break, Ver and Magic, padding runs of 1, 15, 16, 17 and
    40 zeros; tokens ending exactly on a seam and on the stream's last byte.  No stream is handed over."""
    named = seam_streams()
    for name, b in named:
        assert _oracle(b, 1 << 20)[1] == 0, name
    _both(cuda, [b for _, b in named], handed=set())


def test_k2j_phase(cuda):
    """Speculation that never meets the true chain: with a 13-byte first literal the true tokens lie
    on odd stream offsets while chunk and warm-up starts are even, so kj_fix repairs every chunk after
    the first, in order, over several 64-chunk steps.  These streams also hold the most tokens a chunk
    can (one per 2 bytes) and a copy chain tens of thousands deep (D = 11)."""
    for nbytes, jc, nchunk in ((40000, 256, 157), (140000, 1024, 137)):
        ins = []
        for first, parity in ((12, 0), (13, 1)):
            b, start = phase_stream(first, nbytes)
            assert start % 2 == parity and jc % 2 == 0  # (13: tokens on odd offsets; chunk and warm-up starts, multiples of 256, even)
            assert -(-len(b) // jc) == nchunk and nchunk > 64
            want, err = _oracle(b, 1 << 20)
            assert err == 0 and len(want) == first + 6 * ((nbytes - start) // 2)
            ins.append(b)
        assert _need(phase_stream(12, nbytes)[0]) == {40000: 119946, 140000: 419946}[nbytes]
        _run(cuda, ins, jc, handed=set())
        _run(cuda, ins[1:], jc, handed=set())


def test_k2j_bodies_that_look_like_tokens(cuda):
    """Literal bodies of zeros, metas, Len4 headers with huge advances (entries pass through chunks),
    0xff / 0xfc..0xfe and random bytes, with short copies into them: the speculative walks read the
    bodies as tokens, the true chain does not.  No stream is handed over."""
    named = body_streams()
    for name, b in named:
        assert _oracle(b, 1 << 20)[1] == 0, name
    _both(cuda, [b for _, b in named], handed=set())


def test_k2j_copies(cuda):
    """A run of one byte through three maximal Len2 copies, a period of 7, a distance of exactly the
    window and of the window + 1 under a 1 KiB reset (the second is handed over, with the oracle's
    error)."""
    import eazy_amd as ez

    named = copy_streams()
    ins = [b for _, b in named]
    errs = [_oracle(b, 1 << 20)[1] for b in ins]
    assert errs == [0, 0, 0, ez.EOVERFLOW], errs
    _both(cuda, ins, handed={3})


def test_k2j_copy_before_stream_start_reads_zeros(cuda):
    """Stream 1 copies from 2,000 bytes before its own start; the bytes there are stream 0's output
    (0xEE, its slot filled to the last byte), and the copy must read the fresh window's zeros."""
    s0 = HDR + lit(b"\xee" * 3000)
    s1 = HDR + cpy(2000, 30) + lit(b"abc") + cpy(1500, 40) + cpy(33, 33)
    want, err = _oracle(s1, 1 << 20)
    assert err == 0 and want[:30] == bytes(30)
    _both(cuda, [s0, s1], handed=set(), slots={0: 3000}, filler_at=2)
    _both(cuda, [s0, s1], handed=set(), slots={0: 3000}, filler_at=0)


def _tiny(rng):
    return HDR + lit(rb(rng, 40)) + cpy(int(rng.integers(1, 41)), 24)


@pytest.mark.parametrize("count", [1, 2, 64, 65, 1024])
def test_k2j_batch_counts(cuda, count):
    """Batches of 1, 2, 64, 65 and 1,024 streams of 64 output bytes (the per-stream kernels' wave and
    block boundaries), at both chunk sizes (the larger with one stream replaced by a filler, so that
    the count stays the one under test)."""
    rng = np.random.default_rng(200 + count)
    ins = [_tiny(rng) for _ in range(count)]
    assert all(_need(b) == 64 for b in ins)
    _run(cuda, ins, 256, handed=set())
    big = list(ins)
    big[count // 2] = filler()
    _run(cuda, big, 1024, handed=set())


def test_k2j_takes_at_most_1024_streams(cuda):
    """A batch of 1,025 streams does not take K2j even when forced: K2t decodes it."""
    rng = np.random.default_rng(301)
    _run(cuda, [_tiny(rng) for _ in range(1025)], 256, handed=None, last="t")


def test_k2j_empty_streams_and_short_slot(cuda):
    """Empty streams first, in the middle and last; a stream whose slot is one byte short between
    good neighbours: ENOSPC for it alone, the neighbours intact, and it alone handed over."""
    rng = np.random.default_rng(303)
    g = [HDR + lit(rb(rng, 300)) + cpy(200, 150) + cpy(1, 70) for _ in range(4)]
    _both(cuda, [b"", g[0], b"", g[1], b""], handed=set())
    _both(cuda, [b"", b""], handed=set())
    ins = [g[0], g[1], g[2]]
    assert _oracle(g[1], _need(g[1]) - 1)[1] == 2
    _both(cuda, ins, handed={1}, slots={1: _need(g[1]) - 1})
    _both(cuda, ins, handed=set(), slots={1: _need(g[1])})  # (exactly enough: K2j takes it)


def test_k2j_damage_at_seams(cuda):
    """A 16 KiB log stream from the oracle's encoder, truncated at every length within 3 bytes of
    three seams and with every single bit flipped in the four bytes around each: statuses, sizes and
    bytes equal the oracle's (which streams K2j hands over is not prescribed here)."""
    from eazy_amd import synth

    c = orc.compress(1 << 20, 1024, [synth.logs(41, 16384).tobytes()])
    seams = [1024, 2048, 3072]
    assert len(c) > seams[-1] + 64, len(c)
    ins = []
    for m in seams:
        for d in range(-3, 4):
            ins.append(c[: m + d])
        for at in range(m - 2, m + 2):
            for bit in range(8):
                x = bytearray(c)
                x[at] ^= 1 << bit
                ins.append(bytes(x))
    slots = {s: 16384 + 1 + s % 5 for s in range(len(ins))}
    _both(cuda, ins, handed=None, slots=slots)


def test_k2j_extent_hints(cuda):
    """ez_batch.in_bytes / out_bytes: right, one alone, halved and doubled.  Every variant gives the
    exact decoder's (and the oracle's) statuses, sizes and bytes with the sentinels intact: a wrong
    hint costs speed, never memory safety.  An under-stated hint hands every stream to the exact
    decoder (kj_init's guard); a lone hint counts as unknown and an over-stated one only enlarges
    the workspace: K2j decodes those itself."""
    from eazy_amd import synth

    d = synth.logs(43, 4 << 16).tobytes()
    ins = [orc.compress(1 << 20, 1024, [d[k << 16 : (k + 1) << 16]]) for k in range(4)]
    assert all(_need(b) == 1 << 16 for b in ins)
    every = "all"  # (the filler of the larger run too)
    variants = [
        (lambda i, o: {"in_bytes": i, "out_bytes": o}, set()),
        (lambda i, o: {"in_bytes": i}, set()),
        (lambda i, o: {"out_bytes": o}, set()),
        (lambda i, o: {"in_bytes": i, "out_bytes": o // 2}, every),
        (lambda i, o: {"in_bytes": i // 2, "out_bytes": o}, every),
        (lambda i, o: {"in_bytes": 2 * i, "out_bytes": 2 * o}, set()),
    ]
    assert sum(len(b) for b in ins) > SMALL_MAX
    for hints, handed in variants:
        _run(cuda, ins, 1024, handed=handed, hints=hints)  # the four streams as one batch
        _both(cuda, ins, handed=handed, hints=hints)  # ... in batches of 256-byte chunks, and with the filler
