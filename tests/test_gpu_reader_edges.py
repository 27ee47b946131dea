"""The Reader handle (eazy_amd/csrc/ez_reader.hip) on hand-built streams, against the oracle.

The streams of the other Reader tests are compressed log text, random bytes and zero runs cut at
random points: a refill ends wherever the data puts it.  The groups here (tests/reader_streams.py)
place every buffer end, Read end, window edge and threshold of the handle on a chosen byte of a
chosen token: S1-S7 the NewReader(io.Reader) read-ahead (stream_ahead, the only caller of K2j's
continuation mode), W1-W5 the whole decode of NewReaderBytes (reader_ahead, ahead_leave, the staging
window), R1-R4 the Read by Read decode through two device buffers.

The CPU half proves every case first: the oracle's walk of the stream gives the tokens meant, every
cut falls in the token and on the byte the case says (recomputed from the walk), the oracle's decode
gives the plain bytes the builder's model gives (or an error where one is meant), pyoracle's Reader
agrees with the C oracle on every Read, and a coverage test reads the edges back from the cases.

The GPU half holds the handle to the oracle: the same number of Reads, the same (bytes, err) of every
Read, the read-aheads counted per buffer (or whole_decoded) as the case means them, so that no case
passes on another decoder than it claims, the scripted source's running sums equal to the cuts, and
nothing asked of the source after EOF.  A group runs on one handle (Reset / ResetBytes between cases,
buffers kept) and reruns its first case last; one case of each also runs on a fresh handle."""

from functools import lru_cache

import numpy as np
import pytest

import oracle as orc
import pyoracle as po
import reader_streams as rs
from k2_streams import LIT, META_BREAK, META_RESET

EXPECTED_CASES = {"S1": 90, "S2": 32, "S3": 38, "S4": 6, "S5": 15, "S5cap": 2, "S6": 9, "S6eof": 48, "S6ver": 3, "S7": 7,
                  "W1": 9, "W2": 12, "W2cap": 2, "W3": 7, "W4": 9, "R1": 106, "R2": 6, "R3": 6, "R4": 2}
GROUPS = list(EXPECTED_CASES)


# ---------------------------------------------------------------- the CPU half


@lru_cache(None)
def walk(comp):
    """The oracle's walk of a stream: (tokens as reader_streams.Tok, the byte it stopped at, its error).
    Plain positions come from the token lengths, the window from the MetaResets."""
    toks, i, opos = [], 0, 0
    while i < len(comp):
        if comp[i] == 0:
            j = i
            while j < len(comp) and comp[j] == 0:
                j += 1
            toks.append(rs.Tok("z", i, j - i, 0, 0, opos))
            i = j
            continue
        tag, L, j, err = orc.dec_tag(comp, i)
        if err:
            return toks, i, err
        if tag != LIT and L == 0:
            m, ml, j2, err = orc.dec_meta(comp, j)
            if err or j2 + ml > len(comp):
                return toks, i, err or orc.ESHORTBUF
            toks.append(rs.Tok("m", i, j2 + ml - i, 0, m, opos))
            i = j2 + ml
        elif tag == LIT:
            if j + L > len(comp):
                return toks, i, orc.ESHORTBUF
            toks.append(rs.Tok("l", i, j - i, L, 0, opos))
            i, opos = j + L, opos + L
        else:
            D, j2, err = orc.dec_offset(comp, j, L)
            if err:
                return toks, i, err
            toks.append(rs.Tok("c", i, j2 - i, L, D, opos))
            i, opos = j2, opos + L
    return toks, i, 0


def locate(toks, at):
    """(token index, byte of that token) of stream byte `at`; (len(toks), 0) at the tokens' end"""
    for k, t in enumerate(toks):
        if t.start <= at < rs.tok_end(t):
            return k, at - t.start
    assert not toks or at == rs.tok_end(toks[-1]), at
    return len(toks), 0


def all_cases():
    return [c for g in GROUPS for c in rs.GROUPS[g]()]


def _stream(c):
    return c.comp + (c.more or b"")


def test_case_counts():
    assert set(EXPECTED_CASES) == set(rs.GROUPS)
    assert {g: len(rs.GROUPS[g]()) for g in GROUPS} == EXPECTED_CASES
    names = [c.name for c in all_cases()]
    assert len(set(names)) == len(names)
    for g in GROUPS:
        assert all(c.group == g for c in rs.GROUPS[g]())


def test_tokens_are_the_ones_meant():
    """The oracle's walk gives each case's token list; a stream that is meant to end in a damaged or
    cut token stops the walk right after the list."""
    for c in all_cases():
        b = _stream(c)
        toks, end, err = walk(b)
        if err == 0:
            assert tuple(toks) == c.toks, c.name
            assert end == len(b)
        else:
            assert c.plain is None or b[end:] == b"\x80", c.name  # (a meta's first byte alone: consumed, a clean EOF)
            assert tuple(toks) == c.toks[: len(toks)], c.name
            # the tokens meant end where the walk stopped, but for a token built whole and then cut
            assert len(c.toks) - len(toks) <= 1 and end == (rs.tok_end(toks[-1]) if toks else 0), c.name


def test_cuts_fall_where_meant():
    """Every buffer end (mode "s") lies in the token and on the byte the case says; so does the end of
    the upload window (mode "r") of a Read that needs input past it: the input position at the start
    of every Read is pyoracle's."""
    seen = 0
    for c in all_cases():
        toks = walk(_stream(c))[0]
        if c.mode == "s":
            assert c.cuts[-1] == len(c.comp) and list(c.cuts) == sorted(set(c.cuts)), c.name
            cuts = c.cuts[:-1]
            assert len(c.where) == len(cuts), c.name
            for cut, w in zip(cuts, c.where):
                assert locate(toks, cut) == w, (c.name, cut, locate(toks, cut), w)
                seen += 1
        if c.wins:
            r = po.Reader(c.comp)
            r.set(0, 0, *c.flags)
            hit = False
            for k in range(10_000):
                i0, p_len = r.boff + r.i, c.reads[min(k, len(c.reads) - 1)]
                d, err = r.read(p_len)
                if i0 + max(rs.WIN, 2 * p_len + 64) == c.wins[0] and r.boff + r.i >= c.wins[0]:  # (it took all of its window)
                    hit = True
                    assert locate(toks, c.wins[0]) == c.where[0], (c.name, locate(toks, c.wins[0]), c.where)
                    seen += 1
                if err not in (0, orc.EBREAK):
                    break
            assert hit, c.name
    assert seen > 300
    # a Read's result depends on the refill exactly where buffer 1 ends after a meta's first byte
    for c in all_cases():
        if c.mode == "s" and len(c.cuts) > 1:
            toks = walk(c.comp)[0]
            k, off = locate(toks, c.cuts[0])
            assert c.split == (off == 1 and k < len(toks) and toks[k].kind == "m"), c.name
        else:
            assert not c.split
    assert sorted(c.name for c in all_cases() if c.split) == sorted(
        [f"s1-{f}-x1" for f in ("break", "ver", "magic")] + [f"s5-split-{r}" for r, _ in rs.BRK_READS])


def test_oracle_decode_is_the_plain_meant():
    for c in all_cases():
        lens, data = c.want
        if c.plain is not None:
            assert data is c.plain and lens[-1][1] == orc.EOF, (c.name, lens[-1])
        elif c.split:  # (the one-piece decode is the plain meant; this one is the Reader's with the refill there)
            one = rs.pack(rs.run_reads(rs.oracle_reader("s", c.comp).read, c.reads))
            assert one != c.want and one[0][-1][1] == orc.EOF, c.name
        else:
            assert lens[-1][1] not in (orc.OK, orc.EOF, orc.EBREAK), (c.name, lens[-1])
        assert all(n == p or e != 0 for (n, e), p in zip(lens, c.reads + (c.reads[-1],) * len(lens))), c.name


def _py_reader(c):
    if c.mode == "s" or c.more is not None:
        r = po.Reader(src=_stream(c))
        r.set(rs.LIMIT_S if c.mode == "s" else 0, c.cuts[0] if c.split else rs.BUFFER_SIZE, *c.flags)
    else:
        r = po.Reader(c.comp)
        r.set(0, 0, *c.flags)
    return r


def test_pyoracle_agrees_with_the_oracle():
    """pyoracle's Reader gives the C oracle's (bytes, err) at every Read.  Of the streams that decode to
    8 MiB (a byte loop in Python) it runs S4's, which is S7's, and W3's once."""
    s4_big = rs.s4_cases()[-1]
    assert all(c.comp == s4_big.comp and c.plain == s4_big.plain for c in rs.s7_cases())
    assert len({c.comp for c in rs.w3_cases()}) == 1
    for c in all_cases():
        if c.group == "S7" or (c.group == "W3" and c is not rs.w3_cases()[0]):
            continue
        got = rs.pack(rs.run_reads(_py_reader(c).read, c.reads))
        assert got[0] == c.want[0], (c.name, [(k, a, b) for k, (a, b) in enumerate(zip(got[0], c.want[0])) if a != b][:3])
        assert got[1] == c.want[1], c.name


def _form_table(seed):
    return {name: (b, hdr) for name, b, hdr, far in rs.forms(np.random.default_rng(seed))}


def _form_of(table, comp, t):
    for name, (b, hdr) in table.items():
        if comp[t.start : t.start + len(b)] == b and rs.tok_end(t) - t.start == len(b):
            return name
    return None


def _edge_set(cases, table, ends):
    """{(form, byte of the form)} and {(form, "end")} a group's cuts or window ends fall on, read back
    from the streams"""
    got = set()
    for c in cases:
        toks = walk(c.comp)[0]
        k, off = locate(toks, ends(c))
        if k < len(toks):
            got.add((_form_of(table, c.comp, toks[k]), off))
        if off == 0 and k > 0:
            got.add((_form_of(table, c.comp, toks[k - 1]), "end"))
    return got


def test_coverage_read_back_from_the_cases():
    # every form x every header byte, the form's start and end, a literal's body edges: S1 and R1
    for cases, seed, ends in ((rs.s1_cases(), 2101, lambda c: c.cuts[0]), (rs.r1_cases(), 2102, lambda c: c.wins[0])):
        table = _form_table(seed)
        assert list(table) == list(rs.FORMS) and len(table) == 16
        got = _edge_set(cases, table, ends)
        for name, (b, hdr) in table.items():
            need = {(name, x) for x in range(hdr)} | {(name, "end")}
            if len(b) > hdr:
                body = len(b) - hdr
                need |= {(name, hdr), (name, hdr + 1), (name, hdr + body // 2), (name, hdr + body - 1)}
            assert need <= got, (name, sorted(need - got, key=str))
    # the pending literal's length and the output start H + k of the second buffer's read-ahead
    ks, residues = set(), set()
    for c in rs.s2_cases() + rs.s3_cases():
        toks = walk(c.comp)[0]
        k, off = locate(toks, c.cuts[0])
        t = toks[k] if k < len(toks) else None
        pend = rs.tok_end(t) - c.cuts[0] if t is not None and t.kind == "l" and off >= t.hdr else 0
        out = (t.opos + (off - t.hdr if pend else 0)) if t is not None else 0
        resets = [x for x in toks[:k] if x.kind == "m" and x.D == META_RESET]
        bs, w0 = 1 << c.comp[resets[-1].start + 2], resets[-1].opos
        if c.group == "S2":
            ks.add(pend)
        if c.aheads[1] == 1:
            residues.add((min(out - w0, bs) + min(pend, c.cuts[1] - c.cuts[0])) % 16)
    assert ks >= set(rs.S2_K), ks
    assert residues == set(range(16)), residues
    # both sides of every threshold
    one_buffer = {len(c.comp): c.aheads for c in rs.s6_cases() if len(c.cuts) == 1}
    assert one_buffer[rs.STREAM_MIN - 1] == (0,) and one_buffer[rs.STREAM_MIN] == (1,)
    assert {len(c.comp) for c in rs.w1_cases()} == {16_383, 16_384, 16_385}
    for b_len in (16_383, 16_384, 16_385):
        over = {len(c.plain) - (8 * b_len + 4096) for c in rs.w1_cases() if len(c.comp) == b_len}
        assert {0, 1} <= over and max(over) > 3 * (8 * b_len + 4096), over  # (more than 4x the slot: two regrows)
    for cases, first in ((rs.s5_cap_cases(), lambda c: c.cuts[0]), (rs.w2_cap_cases(), lambda c: 0)):
        n = {sum(1 for t in walk(c.comp)[0] if t.kind == "m" and t.D == META_BREAK and t.start >= first(c)): c for c in cases}
        assert set(n) == {rs.BRK_CAP, rs.BRK_CAP + 1}
        assert [(n[k].aheads[-1:], n[k].whole) for k in sorted(n)] in ([((1,), None), ((0,), None)], [((), True), ((), False)])
    # buffer 2 of S4: the output against the slot 8 * n2 + 4096, and the 4x regrows it takes
    slots = set()
    for c in rs.s4_cases():
        toks = walk(c.comp)[0]
        n2, slot = c.cuts[1] - c.cuts[0], 8 * (c.cuts[1] - c.cuts[0]) + 4096
        before = toks[locate(toks, c.cuts[0])[0]].opos
        k, off = locate(toks, c.cuts[1])
        tail = off - toks[k].hdr if off else 0  # (of a literal the buffer ends in)
        made = (toks[k].opos + tail if k < len(toks) else len(c.plain)) - before
        slots.add((min(made - slot, 2), tail > 0, sum(1 for q in (1, 4) if made > q * slot)))
    assert {(0, False, 0), (1, False, 1), (0, True, 0), (1, True, 1), (2, False, 1), (2, False, 2)} == slots, slots
    big = rs.s4_cases()[-1]
    assert 8 * rs.MiB < len(big.plain) - 9000 <= 16 * (8 * rs.S7_N2 + 4096) and len(rs.w3_cases()[0].plain) > 8 * rs.MiB  # (S7, W3)


# ---------------------------------------------------------------- the GPU half


def _first_diff(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return k, g, w
    return min(len(got), len(want)), None, None


def _run_case(r, c):
    """One case on the handle r (an eazy_amd.Reader, reset here): every check of the module's docstring."""
    import eazy_amd as ez

    src = None
    if c.mode == "s":
        pieces = [b - a for a, b in zip((0,) + c.cuts, c.cuts)]
        src = rs.ScriptSrc(c.comp, pieces, c.eof_after)
        r.Reset(src)
        src.reader = r
        r.BlockSizeLimit, r.BufferSize = rs.LIMIT_S, rs.BUFFER_SIZE
    else:
        r.ResetBytes(c.comp)
        r.BlockSizeLimit, r.BufferSize = 0, 0
        if c.mode == "r":
            ez._lib().ez_reader_set_whole(r._h, 0)
        if c.more is not None:  # a Reader set after NewReaderBytes (reader.go:27: a public field)
            src = rs.ScriptSrc(c.more, [len(c.more)])
            r.Reader, r.BufferSize, src.reader = src, rs.BUFFER_SIZE, r
    r.RequireMagic, r.SkipUnsupportedMeta = c.flags
    a0 = r.ahead_count
    whole = []

    def read(n):
        res = r.Read(n)
        if not whole:
            whole.append(r.whole_decoded)
        return res

    got = rs.run_reads(read, c.reads)
    lens, data = rs.pack(got)
    wl, wd = c.want
    assert len(lens) == len(wl), (c.name, "Reads", len(lens), len(wl), lens[-1], wl[-1])
    assert lens == wl, (c.name, "Read (index, got, oracle)", _first_diff(lens, wl))
    if data != wd:
        at = next(k for k in range(min(len(data), len(wd)) + 1) if data[k : k + 1] != wd[k : k + 1])
        raise AssertionError((c.name, "first wrong byte", at, data[at : at + 8].hex(), bytes(wd[at : at + 8]).hex()))
    if c.mode == "s":
        assert src.sums == c.cuts, (c.name, "a piece was clipped", src.log, c.cuts)
        zero = [k for k, (_, m) in enumerate(src.log) if m == 0]
        assert zero in ([], [len(src.log) - 1]), (c.name, src.log)
        counts = src.counts + [r.ahead_count]
        deltas = tuple(counts[j + 1] - counts[j] for j in range(len(src.log)))
        assert deltas[: len(c.aheads)] == c.aheads and not any(deltas[len(c.aheads) :]), (c.name, "read-aheads per buffer", deltas, c.aheads)
        assert not whole[0]
    else:
        assert r.ahead_count == a0, (c.name, "read ahead")
        # (whole_decoded after the first Read, or, where that Read goes on into the second part, at its call for it)
        assert (src.wholes[0] if src is not None else whole[0]) == bool(c.whole), (c.name, "whole_decoded", whole[0])
        if src is not None:
            assert src.at == len(c.more) and src.log[0][1] == len(c.more), (c.name, src.log)


def _run_group(cases):
    import eazy_amd as ez

    r = ez.Reader(b=b"")
    for c in cases + [cases[0]]:
        _run_case(r, c)
    _run_case(ez.Reader(b=b""), cases[len(cases) // 2])


@pytest.mark.gpu
@pytest.mark.parametrize("group", [g for g in GROUPS if g != "S6ver"])
def test_reader_group(cuda, group):
    """S1-S7, W1-W4, R1-R4: see tests/reader_streams.py for what each group places where.  W1 is W5 too:
    its order is small, large, small on one handle, the first case rerun last."""
    _run_group(rs.GROUPS[group]())


@pytest.mark.gpu
def test_reader_version_kept_and_mid_copy(cuda):
    """S6: an unsupported version stays in the handle across Reset (as r.d.Ver does), so the next stream
    is never read ahead; a MetaVer 0 lifts it, and the Read after one that filled p mid-copy finds
    stream_ahead's mid-copy guard.  One handle, the three streams in turn."""
    import eazy_amd as ez

    r = ez.Reader(b=b"")
    for c in rs.s6_ver_cases():
        _run_case(r, c)
