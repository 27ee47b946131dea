"""ez_compress_batch_writes, fresh streams that each receive several Writes, on Write sequences built
byte by byte at every Write edge (tests/k1m_inputs.py) and on the handle's sequences
(tests/k1w_inputs.py) taken as fresh streams.

Two kernels run this path: k1_parse<G, T16, MW = true> (routes 's:parse t16 mw', 's:parse t32 mw'),
whose windows, caps and guards follow the current Write's first and last byte, and the general
kernel's multi-Write variant without a ring ('w:view', 'w:view+gtab'), which re-bases its view of
the input at every Write.  A kernel that is off by one at any of those bounds still writes a stream
that decodes back; only its bytes differ from Go's.  So every sequence's parse by Go is known before
the oracle runs (the unmarked tests prove that on the CPU), and the GPU tests hold every stream's
bytes to the oracle's in slots of exactly the oracle's length, laid back to back at unaligned
offsets between two guards, and every call's route to its name.

The GPU tests are marked one by one: the tests before them run on the CPU."""

import functools

import numpy as np
import pytest

import k1m_inputs as km
import k1w_inputs as kw
import oracle as orc
from k1_inputs import token_at, tokens_of
from test_gpu_k1_hints import FILL, GUARD

MiB = 1 << 20
HEADER = 9  # the magic and the block-size meta

# ------------------------------------------------------------------ the CPU proof

EXPECTED_CASES = {"M1": 34, "M2": 18, "M3": 14, "M4": 21, "M5": 4, "M6": 18, "M7": 4}
EXPECTED_REUSED = {"R1": 29, "R2": 192, "R3": 50, "R4": 81, "R6": 10}  # all of them: 362 of k1w_inputs' 367 (R5 sets positions)
EXPECTED_FIT = {"R1": 29, "R4": 22, "R6": 4}  # the reused cases that k1_parse takes


@pytest.mark.parametrize("g", km.GROUPS)
def test_multi_write_inputs_are_what_they_claim(g):
    """CPU.  For every stream of the group: the C oracle's bytes for the whole stream are its bytes
    Write by Write, concatenated, and pyoracle's (the four long streams of M7: the C oracle alone);
    every stated Write -- the Write under test and each Write after it -- has the intended token list;
    pyoracle's trace of each has the intended accepted matches (branch, acceptor, candidate -- negative:
    in an earlier Write --, bytes found backward and forward), refused candidates and the free-form
    checks; the stream decodes back to the concatenated Writes.  No case is missing: a builder that
    runs out of seeds raises Unbuildable."""
    cases = km.group(g)
    assert len(cases) == EXPECTED_CASES[g], (g, len(cases))
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        comps = kw.oracle_writes(c.block, c.htable, list(c.writes))
        whole = orc.compress(c.block, c.htable, list(c.writes))
        assert comps == c.comps and whole == b"".join(comps), c.name
        assert set(c.want_at) == set(range(c.under, len(c.writes))), c.name
        for j, want in c.want_at.items():
            got = tokens_of(comps[j])[0]
            assert got == want, f"{c.name}: Write {j}"
            assert sum(t[1] for t in got) == len(c.writes[j]), c.name
        if c.c_only:
            assert g == "M7" and c.traces is None
        else:
            py_comps, traces = km.py_traces(c.block, c.htable, c.writes)
            assert py_comps == comps, f"{c.name}: pyoracle and the C oracle differ"
            assert traces == c.traces and km.trace_lacks(c, traces) is None, f"{c.name}: {km.trace_lacks(c, traces)}"
        assert orc.decompress(whole)[0] == c.data, c.name
        if g != "M7":
            assert len(c.data) < 400 and (c.block, c.htable) == (km.BLOCK, km.HTABLE), c.name


def test_reused_handle_sequences_as_fresh_streams():
    """CPU.  The handle's sequences that set no position, as fresh streams at their own block and
    table: the oracle's bytes for the stream are the bytes it gave the handle's Writes one by one
    (where k1w_inputs proved the parse), and the stream decodes back.  55 of them fit half their
    block and 65,536 bytes (k1_parse takes them); the other 307 reach the general kernel."""
    cases = km.reused()
    by = {g: [c for c in cases if c.name.startswith(g + "-")] for g in km.REUSED_GROUPS}
    assert {g: len(v) for g, v in by.items()} == EXPECTED_REUSED and len(cases) == 362
    assert {g: n for g in by if (n := sum(1 for c in by[g] if km.fits(c)))} == EXPECTED_FIT
    assert sum(EXPECTED_FIT.values()) == 55 and len(cases) - 55 == 307
    for c in cases:
        whole = oracle_stream(tuple(c.writes), c.block, c.htable)
        assert whole == b"".join(c.comps), c.name
        assert orc.decompress(whole, cap=max(MiB, 2 * sum(len(p) for p in c.writes)))[0] == b"".join(c.writes), c.name


def _accepts(trace):
    return [e for e in trace if e[0] in ("window", "runlen", "zeros")]


def test_multi_write_inputs_cover_the_edges():
    """CPU.  The counts, positions and lanes the groups are about, read back from the streams' bytes
    and traces (not from the builders' arguments)."""
    # M1: e, the bytes of the repeat that the Write under test still holds: counted backward from the
    # Write's end against the bytes before the next Write's source
    m1 = set()
    for c in km.group("M1"):
        st = c.starts()
        d = c.data
        (ev2,) = _accepts(c.traces[2])
        assert ev2[:2] == ("window", 0) and ev2[3] == 0 and ev2[4] in (8, 40), c.name
        src2 = st[2] + ev2[2]
        e = 0
        while d[st[2] - 1 - e] == d[src2 - 1 - e]:
            e += 1
        n1 = len(c.writes[1])
        acc = _accepts(c.traces[1])
        if e >= 6:
            (ev,) = acc
            assert ev[4] == n1 and ev[4] - ev[3] == e and ev[1] == ev[3], c.name  # the copy ends the Write, nothing backward
            assert tokens_of(c.comps[1])[0][-1] == ("c", e, st[2] - src2 + 0), c.name  # no trailing literal; one distance for both copies
            branch = ev[0]
        else:
            assert not acc, c.name
            branch = "window" if src2 - e < st[1] else "runlen"
        m1.add((branch, e, ev2[4]))
    assert m1 == {(br, e, 40) for br in ("window", "runlen") for e in km.M1_E} | {(br, e, 8) for br in ("window", "runlen") for e in km.M1_E_SHORT}
    # M2: the acceptor's distance from the Write's end, 6 bytes backward, the rest forward to the end
    m2 = set()
    for c in km.group("M2"):
        n1 = len(c.writes[1])
        acc = _accepts(c.traces[1])
        if "insert" in c.name:
            continue
        if "only" in c.name:
            assert not acc and c.want_at[1] == [("l", n1)], c.name
            continue
        (ev,) = acc
        assert ev[1] - ev[3] == 6 and ev[4] == n1, c.name
        m2.add((ev[0], n1 - 4 - ev[1], ev[4] - ev[1]))
    assert m2 == {(br, j, 4 + j) for br in ("window", "runlen") for j in km.M2_J}
    ins = set()
    for c in km.group("M2"):
        if "insert" not in c.name:
            continue
        st = c.starts()
        (ev,) = _accepts(c.traces[1])
        xa, n1 = ev[1], len(c.writes[1])
        cand = st[1] + xa + 1 - st[3]  # position xa + 1 as the fourth Write sees it
        found = [e for e in c.traces[3] if e[0] == "window" and e[2] == cand]
        older = [e for e in c.traces[3] if e[0] == "short" and e[1] == 7 and e[2] < cand]
        assert bool(found) != bool(older), c.name
        assert bool(found) == (xa + 1 + 4 <= n1), c.name
        ins.add((n1 - xa, xa % 32, bool(found)))
    assert ins == {(back, lane, back == 5) for back in (5, 4) for lane in km.M2_LANES}
    # M4: the runs' lengths at a Write's end and at its start
    at_end, at_start, cuts = set(), set(), set()
    for c in km.group("M4"):
        w1 = c.writes[1]
        lead = len(w1) - len(w1.lstrip(b"\0"))
        trail = len(w1) - len(w1.rstrip(b"\0"))
        if "end-the-Write" in c.name:
            (ev,) = _accepts(c.traces[1])
            assert ev[4] == len(w1) and ev[4] - ev[2] == trail and (ev[0] == "zeros") == (trail >= 9), c.name
            at_end.add(trail)
        elif "start-the-Write" in c.name:
            ev = _accepts(c.traces[1])[0]
            assert ev[:3] == ("window", 0, -11) and c.writes[0].endswith(bytes(12)) and ev[3] == 0, c.name  # nothing found backward
            at_start.add(lead)
        else:
            w2 = c.writes[2]
            cuts.add((trail, len(w2) - len(w2.lstrip(b"\0"))))
    assert at_end == set(km.M4_Z) == at_start
    assert cuts == set(km.M4_CUT) | {(a, 8) for a, _ in km.M4_AT_WEND}
    by = {c.name: c for c in km.group("M4")}
    for a, d in km.M4_AT_WEND:  # cand + 8 against the Write's end, zeros beyond it
        c = by[f"M4-candidate+8-at-wend{d:+d}"]
        (ev,) = _accepts(c.traces[1])
        assert ev[2] + 8 - len(c.writes[1]) == d and (ev[0] == "zeros") == (d < 0) and c.writes[2].startswith(bytes(8)), c.name
    # M5: candidate 0, inserted or never
    for c in km.group("M5"):
        j = len(c.writes) - 1
        (ev,) = _accepts(c.traces[j])
        assert c.starts()[j] + ev[2] == 0 and ev[4] - ev[3] == 12, c.name
    assert {len(c.writes[0]) >= 4 for c in km.group("M5")} == {True, False}
    # M6: acceptor, tail, the Write's offset, and the lanes
    m6 = set()
    for c in km.group("M6"):
        (ev,) = _accepts(c.traces[1])
        assert ev[4] - ev[3] == 10 and ev[1] == ev[3], c.name
        m6.add((ev[1], len(c.writes[1]) - ev[4], c.starts()[1]))
    assert m6 == set(km.M6)
    assert {r for r, _, _ in m6} == set(km.M6_R) and {t for _, t, _ in m6} == set(km.M6_T) and {o for _, _, o in m6} == set(km.M6_OFF)
    assert {r % 32 for r, _, _ in m6} >= {0, 15, 16, 31} and {r % 16 for r, _, _ in m6} >= {0, 15}
    # M7: the lengths and where the last repeat lies
    m7 = {c.name: c for c in km.group("M7")}
    assert [len(c.data) for c in m7.values()] == [65536, 65537, 1 << 19, (1 << 19) + 1] and all(len(c.writes) == 3 for c in m7.values())
    for c in list(m7.values())[:2]:
        (ev,) = _accepts(c.traces[2])
        assert len(c.writes[2]) - 4 - ev[1] < 16, c.name  # among the last 16 visited positions
    for c in list(m7.values())[2:]:
        assert c.want_at[2] == [("l", 22), ("c", 12, 20), ("l", 16)] and len(c.writes[2]) == 50, c.name  # both above n - 64


# ------------------------------------------------------------------ device helpers


@functools.lru_cache(maxsize=None)
def oracle_stream(writes: tuple, block: int, htable: int) -> bytes:
    """The oracle's bytes of one fresh stream, computed once per distinct stream."""
    return orc.compress(block, htable, list(writes))


def first_difference(got: bytes, want: bytes) -> str:
    k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
    g = f"{got[k]:#04x}" if k < len(got) else "nothing"
    w = f"{want[k]:#04x}" if k < len(want) else "nothing"
    return f"first difference at byte {k} ({g}, the oracle {w}), the oracle's {token_at(want, k)}"


class WriteBatch:
    """A batch of multi-Write streams on the device: named = [(name, Writes)]."""

    def __init__(self, cuda, named):
        import torch

        self.names = [n for n, _ in named]
        self.streams = [tuple(ws) for _, ws in named]
        in_off, w_idx, w_end, pos = [0], [0], [], 0
        for ws in self.streams:
            for w in ws:
                pos += len(w)
                w_end.append(pos)
            in_off.append(pos)
            w_idx.append(len(w_end))
        self.host = np.frombuffer(b"".join(b"".join(ws) for ws in self.streams), np.uint8).copy()
        self.lens = np.diff(np.array(in_off, np.int64))
        t = lambda a: torch.from_numpy(np.array(a, np.int64)).to(cuda)
        self.data = torch.from_numpy(self.host).to(cuda)
        self.in_off, self.w_idx, self.w_end = t(in_off), t(w_idx), t(w_end)
        self.cuda = cuda

    def slots(self, caps):
        """A CompressedBatch of FILL whose slots have exactly the given capacities, back to back,
        GUARD bytes into the buffer and GUARD bytes before its end."""
        import torch

        import eazy_amd as ez

        so = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + GUARD
        n = len(caps)
        return ez.CompressedBatch(
            torch.full((int(so[-1]) + GUARD,), FILL, dtype=torch.uint8, device=self.cuda),
            torch.from_numpy(so).to(self.cuda),
            torch.full((n,), -1, dtype=torch.int64, device=self.cuda),
            torch.full((n,), -1, dtype=torch.int32, device=self.cuda),
        )

    def compress(self, block, htable, kind, caps):
        """One ez_compress_batch_writes call with the kernel choice `kind` forced -> (route, status,
        sizes, slot offsets, the slots' bytes, the CompressedBatch)."""
        import torch

        import eazy_amd as ez

        out = self.slots(caps)
        ez.select_compress_kernel(kind)
        try:
            cb = ez.compress_batch_writes(self.data, self.in_off, self.w_idx, self.w_end, block, htable, out=out)
            torch.cuda.synchronize()
            route = ez.compress_route_last()
        finally:
            ez.select_compress_kernel("")
        return route, cb.status.cpu().numpy(), cb.sizes.cpu().numpy(), cb.slot_off.cpu().numpy(), cb.slots.cpu().numpy(), cb


def run_writes(cuda, what, named, block, htable, kind, route):
    """One batch of multi-Write streams at one (block, htable) on one forced kind, held to the whole
    bar: the route's name; status 0 and the oracle's size and bytes for every stream, in a slot of
    exactly that size; the guards and the input unchanged; the packed batch decodes back to the
    concatenated Writes.  -> {name: the stream's bytes}."""
    import torch

    import eazy_amd as ez

    wb = WriteBatch(cuda, named)
    want = [oracle_stream(ws, block, htable) for ws in wb.streams]
    got_route, st, sz, off, slots, cb = wb.compress(block, htable, kind, [len(w) for w in want])
    what = f"{what} on {got_route!r} (kind {kind!r}, block {block}, htable {htable}, {len(want)} streams)"
    assert got_route == route, f"{what}: expected route {route!r}"
    bad, out = [], {}
    for s, w in enumerate(want):
        got = slots[off[s] : off[s] + max(int(sz[s]), 0)].tobytes()
        out[wb.names[s]] = got
        if st[s] != 0 or got != w:
            bad.append(f"{wb.names[s]} (stream {s}, Writes of {[len(p) for p in wb.streams[s]][:12]}): status {st[s]}, {sz[s]} bytes, the oracle {len(w)}; {first_difference(got, w)}")
    assert not bad, f"{what}: {len(bad)} of {len(want)} streams differ from the oracle:\n" + "\n".join(bad[:12])
    assert off[0] == GUARD and len(slots) == off[-1] + GUARD
    assert (slots[:GUARD] == FILL).all(), f"{what}: the guard before the first slot was written"
    assert (slots[off[-1] :] == FILL).all(), f"{what}: the guard after the last slot was written"
    assert np.array_equal(wb.data.cpu().numpy(), wb.host), f"{what}: the input was written"
    packed, poff = ez.pack(cb)
    dec, dsz, dst = ez.decompress_batch(packed, poff, wb.in_off)
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0 and dsz.cpu().tolist() == wb.lens.tolist(), f"{what}: decode"
    assert dec[: len(wb.host)].cpu().numpy().tobytes() == wb.host.tobytes(), f"{what}: the decoded bytes are not the Writes"
    return out


def named(cases):
    return [(c.name, tuple(c.writes)) for c in cases]


@functools.lru_cache(maxsize=None)
def small_cases():
    """M1 - M6 and the 55 reused cases that fit half their block: every one under 65,536 bytes."""
    return tuple(c for g in km.SMALL for c in km.group(g)) + tuple(c for c in km.reused() if km.fits(c))


def by_config(cases):
    """{(block, htable): cases}: one batch each, so the batch-wide max_len hint is the longest stream of
    streams that all fit (or all do not fit) half their block."""
    out = {}
    for c in cases:
        out.setdefault((c.block, c.htable), []).append(c)
    return out


def repeated(cases, count):
    """The cases again and again, each copy named, up to `count` streams."""
    out = []
    while len(out) < count:
        k = len(out) // len(cases)
        out += [(f"{c.name} (copy {k})", tuple(c.writes)) for c in cases[: count - len(out)]]
    return out


# ------------------------------------------------------------------ k1_parse and the general kernel


def main_config():
    """((block, table), cases) of the configuration that holds all but 12 of the small cases."""
    return MAIN, by_config(small_cases())[MAIN]


MAIN = (65536, 1024)


def test_small_cases_configs():
    """CPU.  The small cases are 164 streams that k1_parse takes: 152 at block 65,536 (M1 - M6 and 43
    reused cases), and the echoes of 16 and 17 bytes at blocks of 1,024, 4,096 and 16,384, 4 each."""
    cfg = {k: len(v) for k, v in by_config(small_cases()).items()}
    assert cfg == {MAIN: 109 + 43, (1024, 1024): 4, (4096, 1024): 4, (16384, 1024): 4}
    assert all(km.fits(c) for c in small_cases())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("", "s:parse t16 mw"), ("S", "s:parse t32 mw"), ("w", "w:view")], ids=["t16", "t32-32-lanes", "general"])
def test_write_edges_on_every_kernel(cuda, kind, route):
    """M1 - M6 and the 55 reused cases that fit, one batch per (block, table): on k1_parse with the u16
    table (16 lanes per stream), with the u32 table forced (at most 152 streams: 32 lanes per stream,
    split_g32) and on the general kernel's multi-Write variant."""
    for (block, htable), cases in by_config(small_cases()).items():
        run_writes(cuda, "the small cases", named(cases), block, htable, kind, route)


@pytest.mark.gpu
def test_write_edges_on_t32_16_lanes(cuda):
    """The same cases repeated to 8,200 streams with the u32 table forced: above 8,192 streams
    split_g32 gives a stream 16 lanes, k1_parse<16, false, true>.  The route's name does not tell 16
    lanes from 32: the stream count is what selects the kernel.  (The oracle runs once per distinct
    case.)"""
    cfg, cases = main_config()
    run_writes(cuda, "8,200 streams", repeated(cases, 8200), *cfg, "S", "s:parse t32 mw")


GTAB = 8192
GTAB_PARSE_CHANGES = 11  # small cases whose token list at table 8,192 is not the one at 1,024


def test_small_cases_at_table_8192():
    """CPU.  The small cases again at a table of 8,192 entries, where no case was built: the oracle's
    stream still decodes back, and the cases whose parse changes with the table (held by the
    oracle's bytes alone on the GPU) are counted."""
    changed = []
    for c in small_cases():
        big = oracle_stream(tuple(c.writes), c.block, GTAB)
        assert orc.decompress(big)[0] == b"".join(c.writes), c.name
        if tokens_of(big)[0] != tokens_of(oracle_stream(tuple(c.writes), c.block, c.htable))[0]:
            changed.append(c.name)
    print(f"parse changes at table {GTAB}: {len(changed)} of {len(small_cases())}: {changed}")
    assert len(changed) == GTAB_PARSE_CHANGES, changed


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 2100], ids=["a-table-each", "2100-streams"])
def test_write_edges_on_a_global_table(cuda, count):
    """The small cases at table 8,192 on the automatic choice: the general kernel with its tables in
    global scratch.  First every configuration's cases once, a table per stream; then the 152 cases
    of block 65,536 repeated to 2,100 streams, more than the grid's 2,048 blocks (launch_general), so
    a block's table serves a second stream."""
    if count:
        cfg, cases = main_config()
        run_writes(cuda, f"table {GTAB}", repeated(cases, count), cfg[0], GTAB, "", "w:view+gtab")
        return
    for (block, _), cases in by_config(small_cases()).items():
        run_writes(cuda, f"table {GTAB}", named(cases), block, GTAB, "", "w:view+gtab")


@pytest.mark.gpu
def test_reused_cases_beyond_half_the_block(cuda):
    """The 307 reused cases that do not fit half their block (the ring's wrap at every start mod 16,
    the far candidates, the echoes) on the automatic choice at their own block: the ring-less general
    kernel, which reads the same history from the input instead of a ring."""
    cases = [c for c in km.reused() if not km.fits(c)]
    assert len(cases) == 307
    for (block, htable), cs in sorted(by_config(cases).items()):
        run_writes(cuda, f"reused cases at block {block}", named(cs), block, htable, "", "w:view")


@pytest.mark.gpu
def test_table_limits(cuda):
    """M7: 65,536 bytes in 3 Writes (the u16 table's last length), 65,537 (the u32 table by the
    automatic choice; its block is 262,144, since k1_parse takes a stream only in a block of twice
    its length: split_table_words, ez_k1_internal.h), 2^19 (the 20-bit candidate field) and 2^19 + 1
    (the general kernel), each stream alone with its route."""
    for c in km.group("M7"):
        run_writes(cuda, c.name, named([c]), c.block, c.htable, "", km.M7_ROUTES[c.name])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("", "s:parse t16 mw"), ("S", "s:parse t32 mw"), ("w", "w:view")], ids=["t16", "t32", "general"])
def test_order_independence(cuda, kind, route):
    """Every M3 stream between two M1 streams, in two orders: each stream's bytes are the same (and
    the oracle's).  Empty streams and streams of only empty Writes share a wave with live ones: the
    `have` / `live` lanes of a group."""
    m1, m3 = km.group("M1"), list(km.group("M3"))
    a = named([m1[5]] + m3 + [m1[25]])
    b = named([m1[25]] + m3[::-1][3:] + m3[::-1][:3] + [m1[5]])
    assert [n for n, _ in a] != [n for n, _ in b] and sorted(a) == sorted(b)
    got_a = run_writes(cuda, "first order", a, km.BLOCK, km.HTABLE, kind, route)
    got_b = run_writes(cuda, "second order", b, km.BLOCK, km.HTABLE, kind, route)
    assert got_a == got_b


# ------------------------------------------------------------------ short slots


def _inside_a_literal(c, comp):
    """A capacity that ends inside a literal's bytes: the second Write's trailing literal where it
    has one, else the stream's last literal; None for a stream without a literal."""
    toks, at = tokens_of(comp)
    second = len(b"".join(kw.oracle_writes(c.block, c.htable, list(c.writes[:2]))))
    lits = [k for k, t in enumerate(toks) if t[0] == "l" and t[1] > 0]
    if not lits:
        return None
    ends = [(at[k + 1] if k + 1 < len(at) else len(comp)) for k in range(len(toks))]
    k = next((k for k in lits if ends[k] == second and len(c.writes) > 1), lits[-1])
    return ends[k] - 1 - toks[k][1] // 2


# Where a short slot's output ends, per forced kind, as measured on the device.  k1_parse's token
# writer (emit_stream) stops at the last token that fits.  The general kernel writes a literal's tag
# when the tag fits and stops when the literal's bytes do not (put_literal: put_hdr, then put_bytes):
# its output ends at a token boundary or right after a literal's tag, still a prefix of Go's bytes.
SHORT_SLOT_ENDS = {"": {"token"}, "w": {"token", "after a literal's tag"}}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("", "s:parse t16 mw"), ("w", "w:view")], ids=["t16", "general"])
def test_short_slots(cuda, kind, route):
    """M1 and M3 streams in slots of the oracle's length, one byte less, ending inside the second
    Write's trailing literal, and 5 bytes -- held to exactly what test_wide_token_writer_small_slots
    holds single Writes to: a sufficient slot gives status 0 and the exact bytes; a short one
    EZ_ENOSPC, size <= capacity, bytes that are a prefix of the oracle's, and size > 0 when the
    capacity is at least the header plus one token; nothing is written outside the slots.  Where
    the prefix ends is pinned per kernel (SHORT_SLOT_ENDS): the two kernels differ."""
    import eazy_amd as ez

    cases = list(km.group("M1")) + list(km.group("M3"))
    batch, caps, wants = [], [], []
    for c in cases:
        w = oracle_stream(tuple(c.writes), c.block, c.htable)
        for cap in dict.fromkeys([len(w), len(w) - 1, _inside_a_literal(c, w), 5]):
            if cap is not None and 0 <= cap <= len(w):
                batch.append((f"{c.name} in {cap} of {len(w)} bytes", tuple(c.writes)))
                caps.append(cap)
                wants.append(w)
    assert sum(1 for c, w in zip(caps, wants) if c < len(w)) > len(cases) * 2
    wb = WriteBatch(cuda, batch)
    got_route, st, sz, off, slots, _ = wb.compress(km.BLOCK, km.HTABLE, kind, caps)
    assert got_route == route
    bad, ends = [], {}
    for s, (cap, w) in enumerate(zip(caps, wants)):
        n = int(sz[s])
        got = slots[off[s] : off[s] + max(n, 0)].tobytes()
        name = wb.names[s]
        if cap >= len(w):
            if st[s] != 0 or got != w:
                bad.append(f"{name}: status {st[s]}, {n} bytes; {first_difference(got, w)}")
            continue
        toks, at = tokens_of(w)
        first_token_end = at[1] if len(at) > 1 else len(w)
        if st[s] != ez.ENOSPC or not 0 <= n <= cap or got != w[:n]:
            bad.append(f"{name}: status {st[s]} (expected ENOSPC {ez.ENOSPC}), {n} bytes; {first_difference(got, w[:n])}")
        elif cap >= first_token_end and at and n == 0:
            bad.append(f"{name}: nothing written though the header and a token fit")
        elif n in {0, HEADER, len(w), *at}:
            ends.setdefault("token", []).append(name)
        else:
            k = max(j for j in range(len(at)) if at[j] <= n)
            tag = (at[k + 1] if k + 1 < len(at) else len(w)) - at[k] - toks[k][1]  # a literal's bytes before its data
            how = "after a literal's tag" if toks[k][0] == "l" and n == at[k] + tag else "inside a token"
            ends.setdefault(how, []).append(f"{name}: {n} bytes, the oracle's {token_at(w, n)}")
    assert not bad, f"{len(bad)} of {len(caps)} slots on {got_route!r}:\n" + "\n".join(bad[:12])
    assert (slots[:GUARD] == FILL).all() and (slots[off[-1] :] == FILL).all(), "a guard was written"
    assert np.array_equal(wb.data.cpu().numpy(), wb.host), "the input was written"
    print(f"short slots on {got_route!r}: {({k: len(v) for k, v in ends.items()})} of {len(caps)} slots")
    assert set(ends) == SHORT_SLOT_ENDS[kind], f"{got_route!r}: " + "\n".join(f"{k}: {v[:6]}" for k, v in ends.items() if k != "token")
