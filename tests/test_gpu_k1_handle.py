"""The Writer handle (ez_writer_write, ez_writer_write_batch) on Write sequences built byte by
byte at the edges of its own code (tests/k1w_inputs.py): K1L parsing against a ring (RingSrc,
LdsSrc), the general kernel's ring path, the kernels that store a Write into the ring, the table
that lives in the handle from one launch to the next, the routes a call can take.

A handle that is off by one at any of these still writes a stream that decodes back; only its
bytes differ from Go's.  So every sequence's parse by Go is known before the oracle runs (the
unmarked tests prove that on the CPU), and the GPU tests hold every Write's bytes to the oracle's
(oracle/eazy_oracle.c, Write by Write) and the call's route to its name.

The GPU tests are marked one by one: the tests before them run on the CPU."""

import ctypes as C

import numpy as np
import pytest

import k1w_inputs as kw
import oracle as orc
from k1_inputs import token_at, tokens_of
from test_gpu_k1_hints import FILL, GUARD

KiB = 1 << 10
P32 = 1 << 32

# ------------------------------------------------------------------ the CPU proof

EXPECTED_CASES = {"R1": 29, "R2": 192, "R3": 50, "R4": 81, "R5": 5, "R6": 10}


# A Write of 49,151 bytes at position 0 ends one byte before a multiple of these blocks: the ring's
# wrap lies between the first and the second kept byte, which no echo can read (see
# test_handle_echo_cap_of_16_bytes); the same Write at position 9 has its wrap among the bytes read
WRAP_UNREAD = {f"R4-bs{bs}-echo-of-49151-at-0" for bs in (1024, 4096, 16384)}


def _kept(c):
    """An echo case's Write A (the one before the echo): (its start, the ring's first kept position, its end)."""
    a = c.under - 1
    s = c.starts()[a]
    e = s + len(c.writes[a])
    return s, max(s, e - c.block), e


@pytest.mark.parametrize("g", kw.GROUPS)
def test_handle_inputs_are_what_they_claim(g):
    """CPU.  For every sequence of the group: the C oracle's bytes Write by Write are its bytes for
    the whole sequence, and pyoracle's; the tokens of the Write under test are the intended list
    (or hold the named tokens in order); pyoracle's trace of it has the intended accepted matches
    (branch, acceptor, candidate -- negative: in the ring --, bytes found backward and forward), far
    skips and refused candidates; the concatenated stream decodes to the concatenated Writes (not
    where the position is moved between two Writes: the distances then mean other bytes); an echo
    Write's copies read every kept byte but the case's first `unread`, the kept bytes' last 17 and
    both sides of the ring's wrap among them.  No case is missing."""
    cases = kw.group(g)
    assert len(cases) == EXPECTED_CASES[g], (g, len(cases))
    assert len({c.name for c in cases}) == len(cases)
    wraps = 0
    for c in cases:
        comps = kw.oracle_writes(c.block, c.htable, c.writes, c.pos)
        assert comps == c.comps and c.py_comps == comps, f"{c.name}: pyoracle and the C oracle differ"
        got = tokens_of(comps[c.under])[0]
        assert c.tokens is not None or c.named, c.name
        if c.tokens is not None:
            assert got == c.tokens, c.name
        assert kw.holds_in_order(got, c.named), c.name
        assert sum(t[1] for t in got) == len(c.writes[c.under]), c.name
        assert set(c.must) <= {e for e in c.trace if e[0] not in ("far", "short")}, c.name
        assert set(c.far) <= {e[1] for e in c.trace if e[0] == "far"}, c.name
        assert set(c.short) <= {e[1:] for e in c.trace if e[0] == "short"}, c.name
        if not c.pos:
            assert b"".join(comps) == orc.compress(c.block, c.htable, c.writes), c.name
        if set(c.pos) <= {0}:
            assert orc.decompress(b"".join(comps))[0] == b"".join(c.writes), c.name
        if c.unread is not None:
            s, k0, e = _kept(c)
            assert e == c.starts()[c.under], c.name
            reads, at = kw.ring_reads(c), k0 + c.unread
            for lo, hi in reads:  # the union of the ranges read, from the first byte that must be
                if lo <= at:
                    at = max(at, hi)
            assert at == e, f"{c.name}: the echo's copies read {reads[:4]} ..., not every kept byte from {k0 + c.unread} to {e}"
            L = len(c.writes[c.under - 1])
            assert c.unread <= (kw.ECHO_CAP if kw.echo_cap_reachable(c.block, L) else kw.echo_plan(c.block, L)[1]), c.name
            assert c.unread == 0 or c.unread <= e - k0 - 17, c.name
            wrap = e - e % c.block  # the last position of slot 0 the Write holds
            if k0 < wrap < e:
                assert (wrap - 1 >= k0 + c.unread) != (c.name in WRAP_UNREAD), f"{c.name}: the ring's wrap lies in the bytes that are not read"
                wraps += 1
    if g == "R4":
        assert wraps == 39


def test_handle_echo_cap_of_16_bytes():
    """CPU.  The echo's copies read every kept byte except at most the first 16 in 52 of the 72
    echo cases, among them every one whose ring is not full to the last byte or two at a block of 16
    KiB or more: the Writes of 49,151 .. 49,153 bytes kept whole in a 64 KiB ring are read from their
    first or second byte on (three copies of about 16 KiB), the Write of 16,383 bytes in a 16 KiB
    ring by 963 copies of 17 bytes.  The other 20 are not built to it (k1w_inputs.echo_cap_reachable has the
    reason: as many copies as the table has entries, or more): a full ring of 16,384 bytes is read
    from byte 32 on, one of 65,535 or 65,536 bytes from byte 127 or 128 on."""
    echoes = [c for c in kw.group("R4") if c.unread is not None]
    assert len(echoes) == 72
    relaxed = {}
    for c in echoes:
        L = len(c.writes[c.under - 1])
        if c.unread > kw.ECHO_CAP:
            assert not kw.echo_cap_reachable(c.block, L), c.name
            relaxed.setdefault((c.block, c.unread), set()).add(L)
    assert relaxed == {
        (16384, 32): {16384, 16385, 32773, 49151, 49152, 49153},
        (65536, 127): {65535},
        (65536, 128): {65536, 65537, 131077},
    }
    whole = {c.name: c.unread for c in echoes if c.block == 65536 and 49151 <= len(c.writes[c.under - 1]) <= 49153}
    assert sorted(whole.values()) == [0, 0, 0, 0, 1, 1], whole


def _accepts(c):
    return [e for e in c.trace if e[0] in ("window", "runlen")]


def test_handle_inputs_cover_the_edges():
    """CPU.  The offsets, splits, residues and lengths the groups are about, read back from the
    cases' bytes, tokens and traces (not from the builders' arguments)."""
    r1 = kw.group("R1")
    # R1: a 40-byte source k bytes before the Write: k from the copies' lengths, then held against the bytes
    ks = set()
    for c in r1:
        if "source" in c.name:
            t = tokens_of(c.comps[c.under])[0]
            copies = [u[1] for u in t if u[0] == "c"]
            k = copies[0] if len(copies) == 2 else 40 - copies[0]
            p, h = c.writes[c.under], c.writes[c.under - 1]
            x = t[0][1] if k >= 6 else t[0][1] - k
            assert p[x : x + 40] == h[len(h) - k :] + p[: 40 - k], c.name
            assert copies == ([k, 40 - k] if k >= 6 else [40 - k]) and {u[2] for u in t if u[0] == "c"} == {x + k}, c.name  # never one copy of 40
            ks.add(k)
    assert ks == set(kw.R1_K)
    lures = {}
    for c in r1:
        if "lure" in c.name:
            (_, i, cand, ist, iend), = _accepts(c)
            p, h = c.writes[c.under], c.writes[c.under - 1]
            assert i - ist == cand and p[ist - 12 : ist] == h[-12:], c.name  # found backward to position 0; the ring's 12 before it
            lures[cand] = iend - ist
    assert lures == {y: y + 12 for y in kw.R1_LURE_Y}
    assert {_accepts(c)[0][2] for c in r1 if "candidate" in c.name} == set(kw.R1_CAND_Y)
    y0 = [c for c in r1 if c.name == "R1-candidate-at-0"][0]
    assert y0.writes[1][_accepts(y0)[0][1] - 1] == y0.writes[0][-1]  # the ring's last byte before the plant, not found
    # R2: (start mod 16, bytes of the source before the wrap), by block and by the prefix Write's kernel
    seen = {}
    for c in kw.group("R2"):
        (_, i, cand, ist, iend), = _accepts(c)
        start = c.starts()[c.under]
        assert iend - ist == 48 and (start + cand) // c.block == 0 and (start + cand + 47) // c.block == 1, c.name
        seen.setdefault((c.block, len(c.writes[0]) >= 16), set()).add((start % 16, c.block - (start + cand) % c.block))
    for bs in (1024, 65536):
        for lp in (False, True):
            assert seen[(bs, lp)] == {(r, s) for r in kw.R2_RES for s in kw.R2_SPLIT}
    # R3: the first candidate of the plant, relative to the staged extent, and what became of it
    r3 = {}
    for c in kw.group("R3"):
        P = 0 if "back" in c.name else 5
        ev = [e for e in c.trace if e[1] == P][0]
        cand = ev[2] if ev[0] != "far" else None
        r3.setdefault(c.block, []).append((ev[0], None if cand is None else cand + min(c.block, kw.R3_RL), P))
    assert sorted(d for k, d, _ in r3[65536] if k == "window") == sorted(2 * list(kw.R3_D))
    assert {e[4] - e[3] for c in kw.group("R3") if c.block == 65536 for e in _accepts(c)} == {40, 200}
    for bs in (32768, 16384):
        assert sorted((k, d) for k, d, P in r3[bs] if P == 5 and k != "far") == sorted([("short", d) for d in kw.R3_D if 0 <= d < 11] + [("window", 24)])
        assert sum(1 for k, d, P in r3[bs] if P == 5 and k == "far") == sum(1 for d in kw.R3_D if d < 0)
        assert sorted((k, d) for k, d, P in r3[bs] if P == 0) == sorted([("short", 1), ("short", 0), ("far", None)])
    # R4: the lengths, as the Write under test and as the Write an echo follows
    r4 = kw.group("R4")
    assert [len(c.writes[c.under]) for c in r4 if c.unread is None] == list(kw.R4_LEN)
    echoes = {(c.block, len(c.writes[c.under - 1]), c.starts()[c.under - 1] % 16) for c in r4 if c.unread is not None}
    assert echoes == {(bs, L, r) for bs in kw.R4_BS for L in [bs - 1, bs, bs + 1, 2 * bs + 5, 16, 17, 49151, 49152, 49153] for r in kw.R4_RES}
    # R5: the positions
    r5 = {c.name: c for c in kw.group("R5")}
    ends = {n: c.starts()[c.under] + len(c.writes[c.under]) for n, c in r5.items()}
    assert ends["R5-ends-at-2^32"] == P32 and ends["R5-ends-at-2^32+1"] == P32 + 1
    assert r5["R5-starts-at-2^32"].starts()[1] == P32
    assert r5["R5-jump-2^28+100"].starts()[1] == 64 + (1 << 28) + 100 and r5["R5-jump-and-back"].starts()[2] == 64
    # R6: the calls
    r6 = [[[len(c.writes[j]) for j in call] for call in c.calls] for c in kw.group("R6")]
    first = [calls[0] for calls in r6]
    assert {len(f) for f in first} == {2, 3, 4}
    assert any(0 in f for f in first) and any(5 in f for f in first)
    assert {len(f) for f in first if min(f) >= 16 and max(f) <= kw.LDS_WRITE} == {2, 3, 4} == {len(f) for f in first if max(f) > kw.LDS_WRITE}
    assert sum(1 for c in kw.group("R6") if c.block == 1024 and sum(len(c.writes[j]) for j in c.calls[0]) > 1024 and len(c.calls) == 2) == 2


# ------------------------------------------------------------------ the routes


def expected_route(htable, forced_w, start, lens):
    """The route of one handle call: K1L takes it when every Write has 16 bytes or more
    and ends at or before 2^32 (table of at most 4,096 entries, version 0, nothing forced); else the
    general kernel takes all of it in one launch."""
    at, k1l = start, not forced_w and htable <= 4096
    for n in lens:
        k1l = k1l and 16 <= n < (1 << 26) and at + n <= P32
        at += n
    if k1l:
        if len(lens) > 1:
            return "hl:batch zero-copy" if max(lens) <= kw.LDS_WRITE else "hl:batch staged"
        return "hl:lds" if lens[0] <= kw.LDS_WRITE else "hl:global"
    gtab = "+gtab" if htable > 4096 else ""
    if len(lens) > 1:
        return "hw:multi" + gtab
    return ("hw:pl" if max(lens[0], 1) <= 16 * KiB else "hw:view") + gtab


def test_expected_route_thresholds():
    """CPU.  The thresholds of expected_route are the issue's: 15 | 16, 49,152 | 49,153, 2^32,
    the table of 4,096, 16 KiB of LDS staging in the general kernel."""
    assert [expected_route(1024, False, 0, [n]) for n in (0, 15, 16, 49152, 49153)] == ["hw:pl", "hw:pl", "hl:lds", "hl:lds", "hl:global"]
    assert expected_route(1024, False, P32 - 37, [37]) == "hl:lds" and expected_route(1024, False, P32 - 36, [37]) == "hw:pl"
    assert expected_route(8192, False, 0, [100]) == "hw:pl+gtab" and expected_route(8192, False, 0, [16385]) == "hw:view+gtab"
    assert expected_route(1024, True, 0, [16384]) == "hw:pl" and expected_route(1024, True, 0, [16385]) == "hw:view"
    assert expected_route(1024, False, 0, [16, 49152]) == "hl:batch zero-copy" and expected_route(1024, False, 0, [16, 49153]) == "hl:batch staged"
    assert expected_route(1024, False, 0, [40, 5, 60]) == "hw:multi" and expected_route(8192, False, 0, [40, 60]) == "hw:multi+gtab"


# ------------------------------------------------------------------ device helpers


def first_difference(got: bytes, want: bytes) -> str:
    k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
    g = f"{got[k]:#04x}" if k < len(got) else "nothing"
    w = f"{want[k]:#04x}" if k < len(want) else "nothing"
    return f"first difference at byte {k} ({g}, the oracle {w}), the oracle's {token_at(want, k)}"


class Handles:
    """One handle per (block, htable), made on first use and freed together."""

    def __init__(self):
        import eazy_amd as ez

        self.ez, self.L, self.h = ez, ez._lib(), {}
        self.L.ez_writer_set_position.argtypes = [C.c_void_p, C.c_int64]

    def get(self, block, htable):
        if (block, htable) not in self.h:
            h = C.c_void_p()
            assert self.L.ez_writer_new(block, htable, 0, C.byref(h)) == 0
            self.h[(block, htable)] = h
        return self.h[(block, htable)]

    def free(self):
        for h in self.h.values():
            self.L.ez_writer_free(h)
        self.h = {}


@pytest.fixture(scope="module")
def handles(cuda):
    hs = Handles()
    yield hs
    hs.free()


_PAD = np.random.default_rng(20).integers(1, 256, 49153, dtype=np.uint8).tobytes()
_oracle = {}


def sequence(c, pad, htable):
    """The case's Writes with the one under test padded with trailing filler to `pad` bytes, and the
    oracle's bytes for each at that table size."""
    key = (c.name, pad, htable)
    if key not in _oracle:
        ws = list(c.writes)
        if len(ws[c.under]) < pad:
            ws[c.under] = ws[c.under] + _PAD[: pad - len(ws[c.under])]
        _oracle[key] = (ws, kw.oracle_writes(c.block, htable, ws, c.pos))
    return _oracle[key]


def run_case(hs, c, delivery, kind, htable=None, pad=0):
    """One sequence on its configuration's handle, reset first.  delivery: "write" (one
    ez_writer_write per Write), "batch" (the sequence in one ez_writer_write_batch), "calls" (the
    case's own calls).  Every call's output buffer is ez_compress_bound long with a guard after it;
    every Write's status, size and bytes are the oracle's, the guard and the input are unchanged, and
    the last call's route is the expected one.  -> (the Writes' bytes, the last call's route)."""
    ez, L = hs.ez, hs.L
    htable = htable or c.htable
    ws, want = sequence(c, pad, htable)
    h = hs.get(c.block, htable)
    assert L.ez_writer_reset(h) == 0
    calls = {"write": [[j] for j in range(len(ws))], "batch": [list(range(len(ws)))], "calls": c.calls}[delivery]
    what = f"{c.name} ({delivery}, kind {kind!r}, block {c.block}, htable {htable}, padded to {pad})"
    starts, outs, route = c.starts(), [], ""
    ez.select_compress_kernel(kind)
    try:
        for call in calls:
            for j in call:
                if j in c.pos:
                    assert len(call) == 1 or j == call[0]
                    assert L.ez_writer_set_position(h, c.pos[j]) == 0
            lens = [len(ws[j]) for j in call]
            src = np.frombuffer(b"".join(ws[j] for j in call) + b"\x00", np.uint8).copy()
            keep = src.copy()
            cap = sum(ez.compress_bound(n) for n in lens)
            out = np.full(cap + GUARD, FILL, np.uint8)
            sp, op = C.cast(src.ctypes.data, C.c_char_p), C.c_void_p(out.ctypes.data)
            if len(call) == 1:
                n = C.c_size_t()
                st = L.ez_writer_write(h, sp, lens[0], op, cap, C.byref(n))
                ends = [n.value]
            else:
                e = np.cumsum(lens).astype(np.uint64)
                oe = np.zeros(len(call), np.uint64)
                st = L.ez_writer_write_batch(h, sp, C.c_void_p(e.ctypes.data), len(call), op, cap, C.c_void_p(oe.ctypes.data))
                ends = [int(v) for v in oe]
            route = ez.compress_route_last()
            assert st == 0, f"{what}: call {call} on {route!r}: status {st}"
            at = 0
            for j, end in zip(call, ends):
                got = out[at:end].tobytes()
                assert got == want[j], (
                    f"{what}: Write {j} of {len(ws)} ({len(ws[j])} bytes at position {starts[j]}) on {route!r}: {end - at} bytes, "
                    f"the oracle {len(want[j])}; {first_difference(got, want[j])}"
                )
                outs.append(got)
                at = end
            assert (out[cap:] == FILL).all(), f"{what}: call {call}: the guard after the output was written"
            assert np.array_equal(src, keep), f"{what}: call {call}: the input was written"
            if kind == "" or kind == "w":
                exp = expected_route(htable, kind == "w", starts[call[0]], lens)
                assert route == exp, f"{what}: call {call} took {route!r}, expected {exp!r}"
    finally:
        ez.select_compress_kernel("")
    return outs, route


def run_group(hs, cases, delivery, kind, htable=None, pad=0):
    """Every case of the group, then on every handle the group used (one per block) its first case
    again: after all the others and ez_writer_reset it gives the same bytes, so nothing a case leaves
    in a handle reaches a later one.  -> the routes of the cases' last calls."""
    routes = set()
    first = {}
    for c in cases:
        outs, route = run_case(hs, c, delivery, kind, htable, pad)
        first.setdefault(c.block, (c, outs))
        routes.add(route)
    for c, outs in first.values():
        again, _ = run_case(hs, c, delivery, kind, htable, pad)
        assert again == outs, f"{c.name} again after the group: the handle kept something across ez_writer_reset"
    return routes


DELIVERIES = [("write", ""), ("batch", ""), ("write", "w"), ("batch", "w")]
delivery = pytest.mark.parametrize("how,kind", DELIVERIES, ids=["write-auto", "batch-auto", "write-general", "batch-general"])


def _reached(how, kind):
    """The routes a group of short sequences of Writes of 16 bytes or more must reach."""
    if how == "write":
        return {"hw:pl"} if kind == "w" else {"hl:lds"}
    return {"hw:multi"} if kind == "w" else {"hl:batch zero-copy"}


# ------------------------------------------------------------------ R1 - R6


@pytest.mark.gpu
@delivery
def test_handle_write_start(handles, how, kind):
    """R1: a 40-byte source that begins 1 .. 24 bytes before the Write (two copies at one distance,
    never one of 40); a repeat found at candidates 0 .. 9 with the ring's last 12 bytes in front of it
    (nothing found backward across the Write's start); candidates at -24 .. -7 and 0 .. 9 (the three
    branches of RingSrc::around, both sides of each comparison)."""
    assert run_group(handles, kw.group("R1"), how, kind) == _reached(how, kind)


@pytest.mark.gpu
@delivery
def test_handle_ring_end(handles, how, kind):
    """R2: a 48-byte source across the ring's last and first slot with 1 .. 31 bytes before the wrap,
    the Write at every residue mod 16 that ring_at's byte loop and the staging loop distinguish, the
    history written by the general kernel (a prefix under 16 bytes) and by K1L; blocks of 1,024 and
    65,536.  In one call a prefix under 16 bytes sends the sequence to the multi-Write general kernel."""
    routes = run_group(handles, kw.group("R2"), how, kind)
    assert routes == ({"hl:batch zero-copy", "hl:batch staged", "hw:multi"} if (how, kind) == ("batch", "") else _reached(how, kind))


@pytest.mark.gpu
@delivery
def test_handle_staged_extent(handles, how, kind):
    """R3: candidates at -rl - 24 .. -rl + 24 around the ring bytes K1L stages in LDS (rl = 32,768 of a
    65,536-byte block: LdsSrc::around and bytes48 switch to the ring in HBM), copies of 40 and 200 bytes;
    blocks of 32,768 and 16,384, where rl is the block and the same offsets meet the far skip and
    trim 1."""
    assert run_group(handles, kw.group("R3"), how, kind) == _reached(how, kind)


@pytest.mark.gpu
@delivery
def test_handle_lengths_and_ring_store(handles, how, kind):
    """R4: Writes of 0 .. 17 and 49,151 .. 49,153 bytes (the general kernel | K1L at 16, K1L staged in
    LDS with the ring store fused | K1L from global memory with k1_ring_store past 49,152), and an
    echo Write after Writes of bs - 1 .. 2 bs + 5 and 16 .. 49,153 bytes at residues 0 and 9, blocks of
    1 KiB .. 64 KiB, whose copies read what each ring store kept."""
    routes = run_group(handles, kw.group("R4"), how, kind)
    if how == "write":
        assert routes == ({"hw:pl", "hw:view"} if kind == "w" else {"hw:pl", "hl:lds", "hl:global"})
    else:
        assert routes == ({"hw:multi"} if kind == "w" else {"hw:multi", "hl:batch zero-copy", "hl:batch staged"})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["", "w"], ids=["auto", "general"])
def test_handle_positions_and_clamp(handles, kind):
    """R5: a Write that ends at 2^32 is K1L's and one byte later the general kernel's, by route name;
    a Write at 2^32 after a K1L Write that ended there; a jump of 2^28 + 100 with ring and table kept
    (every entry clamped, none written back), and the position set back to where they are near again."""
    by = {}
    for c in kw.group("R5"):
        by[c.name] = run_case(handles, c, "write", kind)[1]
    run_case(handles, kw.group("R5")[0], "write", kind)
    if kind == "":
        assert by == {"R5-ends-at-2^32": "hl:lds", "R5-ends-at-2^32+1": "hw:pl", "R5-starts-at-2^32": "hw:pl", "R5-jump-2^28+100": "hl:lds", "R5-jump-and-back": "hl:lds"}
    else:
        assert set(by.values()) == {"hw:pl"}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["", "w"], ids=["auto", "general"])
def test_handle_several_writes_in_one_call(handles, kind):
    """R6: calls of 2 .. 4 Writes: all of 16 .. 49,152 bytes (K1L, zero-copy), one longer (K1L, staged
    copies), one of 0 or 5 bytes (the multi-Write general kernel); with a block of 1,024 a call longer
    than the window, then an echo Write in a call of its own.  out_ends are the oracle's ends."""
    by = {}
    for c in kw.group("R6"):
        by[c.name] = run_case(handles, c, "calls", kind)[1]
    run_case(handles, kw.group("R6")[0], "calls", kind)
    got = {n[3:]: r for n, r in by.items()}
    if kind == "w":
        assert {r for n, r in got.items() if not n.startswith("bs1024")} == {"hw:multi"}
        assert {r for n, r in got.items() if n.startswith("bs1024")} == {"hw:pl"}  # the echo's own call
        return
    assert got == {
        "k2-zero-copy": "hl:batch zero-copy", "k3-zero-copy": "hl:batch zero-copy", "k4-zero-copy": "hl:batch zero-copy",
        "k2-staged": "hl:batch staged", "k3-staged": "hl:batch staged", "k4-staged": "hl:batch staged",
        "k3-with-empty-Write": "hw:multi", "k3-with-5-byte-Write": "hw:multi",
        "bs1024-call-longer-than-window-multi": "hl:lds", "bs1024-call-longer-than-window-k1l": "hl:lds",
    }


# ------------------------------------------------------------------ other tables, other stagings


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["write", "batch"])
@pytest.mark.parametrize("g", ["R1", "R2"])
def test_handle_global_table(handles, g, how):
    """R1 and R2 with a table of 8,192 entries: the general kernel on a ring with its table in
    global memory (the handle's own), one Write per launch and the multi-Write form."""
    routes = run_group(handles, kw.group(g), how, "", htable=8192)
    assert routes == ({"hw:pl+gtab"} if how == "write" else {"hw:multi+gtab"})


@pytest.mark.gpu
@pytest.mark.parametrize(
    "kind,pad,htable,route",
    [("", 49153, None, "hl:global"), ("w", 49153, None, "hw:view"), ("w", 16385, None, "hw:view"), ("", 16385, 8192, "hw:view+gtab")],
    ids=["k1l-global", "general-49153", "general-16385", "general-16385-global-table"],
)
@pytest.mark.parametrize("g", ["R1", "R2", "R3"])
def test_handle_write_read_from_global_memory(handles, g, kind, pad, htable, route):
    """R1 - R3 with the Write under test padded with trailing filler to 49,153 bytes -- K1L reads it
    from global memory (RingSrc alone, no LDS image; the token writer and the ring store are launches
    of their own), the general kernel forced takes its global view on a ring -- and to 16,385 bytes,
    just out of the general kernel's LDS staging (there also with a table of 8,192 entries in the
    handle's global memory)."""
    assert run_group(handles, kw.group(g), "write", kind, htable=htable, pad=pad) == {route}
