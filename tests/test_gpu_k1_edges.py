"""K1, the encoder, on inputs built byte by byte at its parse edges (tests/k1_inputs.py), on
every route.

A kernel that is off by one at a judgement cap, a window lane, a ring trim or a token width
still writes a valid stream that decodes back; only its bytes differ from Go's.  So every case
sits on one such edge, its parse by Go is known before the oracle runs (the first test proves
that on the CPU), and the GPU tests compare bytes with the oracle, stream by stream, in slots
of exactly the oracle's length laid back to back at unaligned offsets between two guards: a
store past a stream's end corrupts its neighbour or a guard.

The GPU tests are marked one by one: the first test runs on the CPU."""

import functools

import numpy as np
import pytest

import k1_inputs as ki
import oracle as orc
from test_gpu_k1_hints import FILL, GUARD, DevBatch

MiB, KiB = 1 << 20, 1 << 10

# ------------------------------------------------------------------ the CPU proof


@pytest.mark.parametrize("g", ki.GROUPS)
def test_k1_edge_inputs_are_what_they_claim(g):
    """CPU.  For every case of the group: pyoracle's bytes are the C oracle's; the oracle's
    tokens are the intended list; pyoracle's trace shows the intended branch, acceptor,
    candidate and backward / forward counts of every accepted match (of the named ones where a
    long stream's sparse events are held by their tokens alone), the intended far skips and
    the candidates that must be looked at and refused.  No case is missing: a builder that
    runs out of seeds raises.  (k1_inputs.make() demands the same of a seed before it returns a
    case, so this test fails mostly through Unbuildable and the case counts; what is checked
    independently of the builders is in test_k1_edge_inputs_cover_the_edges.)"""
    cases = ki.group(g)
    assert len(cases) == EXPECTED_CASES[g], (g, len(cases))
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        comp = orc.compress(c.block, c.htable, [c.data])
        assert c.py_comp == comp, f"{c.name}: pyoracle and the C oracle differ"
        assert ki.tokens_of(comp)[0] == c.tokens, c.name
        acc = [e for e in c.trace if e[0] not in ("far", "short")]
        if c.events is not None:
            assert acc == c.events, c.name
        assert set(c.must) <= set(acc), c.name
        assert set(c.far) <= {e[1] for e in c.trace if e[0] == "far"}, c.name
        assert set(c.short) <= {e[1:] for e in c.trace if e[0] == "short"}, c.name
        assert orc.decompress(comp)[0] == c.data, c.name
        if not g.startswith(("H", "I", "J", "Glong")):
            assert len(c.data) <= 4096, c.name


EXPECTED_CASES = {"A": 554, "B": 59, "C": 43, "D": 15, "E": 91, "F": 69, "G": 34, "Glong": 5, "H1024": 22, "H4096": 22, "I": 12, "J": 17}


def _found(g, branch=None):
    """{(backward, forward)} over the group's accepted matches (of one branch)."""
    return {(e[1] - e[3], e[4] - e[1]) for c in ki.group(g) for e in (c.events or c.must) if branch in (None, e[0])}


def test_k1_edge_inputs_cover_the_edges():
    """CPU.  The counts the issue asks for are there, read back from the traces: forward 6..300
    in the window (and none for 5), backward 0..40 and 71..73, 135..137 with nothing and with
    done stopping them, every branch, both zero-token thresholds, the empty literal, the cut
    and the trims."""
    fw = {f for b, f in _found("A", "window") if b == 0}
    assert set(range(6, 301)) | {379, 380, 381} <= fw and 5 not in fw
    assert [c.tokens for c in ki.group("A") if c.name == "A-len5"][0] == [("l", 26), ("c", 8, 16), ("l", 3 + 5 + 11)]  # no second copy
    bw = {b for c in ki.group("B") if "done" not in c.name for b in [c.events[-1][1] - c.events[-1][3]]}
    assert bw == set(ki.B_FREE)
    for c in ki.group("B"):
        if "done" in c.name:
            ev = c.events[-1]
            assert ev[3] == c.events[-2][4] and c.data[ev[3] - 1] == c.data[ev[2] - (ev[1] - ev[3]) - 1], c.name  # only done stops it
    branches = {e[0] for g in ("C", "D", "E", "H1024") for c in ki.group(g) for e in c.events}
    assert branches == {"window", "runlen", "zeros", "cut"}
    assert any(("l", 0) in c.tokens for c in ki.group("E"))
    zt = {c.name: any(t[0] == "c" and t[2] == 0 for t in c.tokens) for c in ki.group("E") if c.name.startswith("E-zeros") and "after" not in c.name}
    assert zt["E-zeros8-middle"] and not zt["E-zeros7-middle"] and zt["E-zeros9-end"] and not zt["E-zeros8-end"]
    for bs in (1024, 4096):
        cut = [c for c in ki.group(f"H{bs}") if "in-literal" in c.name]
        assert [[t for t in c.tokens if t[0] == "c"][1][1:] for c in cut] == [(10, bs - 9), (8, bs - 8), (7, bs - 7)]
        assert sum(len(c.far) for c in ki.group(f"H{bs}")) == 2


# ------------------------------------------------------------------ device helpers


@functools.lru_cache(maxsize=None)
def oracle_bytes(data: bytes, block: int, htable: int) -> bytes:
    return orc.compress(block, htable, [data])


def first_difference(got: bytes, want: bytes) -> str:
    k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
    g = f"{got[k]:#04x}" if k < len(got) else "nothing"
    w = f"{want[k]:#04x}" if k < len(want) else "nothing"
    return f"first difference at byte {k} ({g}, the oracle {w}), the oracle's {ki.token_at(want, k)}"


def run_route(cuda, what, named, block, htable, kind, max_len, route=None):
    """One batch on one route, held to the whole bar: the route's name; status 0, the oracle's
    size and bytes for every stream in a slot of exactly that size, the slots back to back
    between two guards of FILL; the guards and the input unchanged; the packed batch decodes
    back to the input on the automatic K2.  named: [(name, bytes)].  -> the route taken."""
    import torch

    import eazy_amd as ez

    names = [n for n, _ in named]
    bufs = tuple(b for _, b in named)
    dev = DevBatch(cuda, bufs)
    want = [oracle_bytes(b, block, htable) for b in bufs]
    so = torch.from_numpy(np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)).to(cuda)
    out = dev.guarded(so)
    ez.select_compress_kernel(kind)
    try:
        cb = ez.compress_batch(dev.data, dev.off, block, htable, max_len=max_len, out=out)
        torch.cuda.synchronize()
        got_route = ez.compress_route_last()
    finally:
        ez.select_compress_kernel("")
    what = f"{what} on {got_route!r} (kind {kind!r}, max_len {max_len}, block {block}, htable {htable})"
    if route is not None:
        assert got_route == route, f"{what}: expected route {route!r}"
    st, sz, off, slots = cb.status.cpu().numpy(), cb.sizes.cpu().numpy(), cb.slot_off.cpu().numpy(), cb.slots.cpu().numpy()
    bad = []
    for s, w in enumerate(want):
        got = slots[off[s] : off[s] + max(int(sz[s]), 0)].tobytes()
        if st[s] != 0 or got != w:
            bad.append(f"{names[s]} (stream {s}, {len(bufs[s])} bytes): status {st[s]}, {sz[s]} bytes, the oracle {len(w)}; {first_difference(got, w)}")
    assert not bad, f"{what}: {len(bad)} of {len(want)} streams differ from the oracle:\n" + "\n".join(bad[:12])
    assert off[0] == GUARD and len(slots) == off[-1] + GUARD
    assert (slots[:GUARD] == FILL).all(), f"{what}: the guard before the first slot was written"
    assert (slots[off[-1] :] == FILL).all(), f"{what}: the guard after the last slot was written"
    assert np.array_equal(dev.data.cpu().numpy(), dev.host), f"{what}: the input was written"
    packed, poff = ez.pack(cb)
    dec, dsz, dst = ez.decompress_batch(packed, poff, dev.off)
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0 and dsz.cpu().tolist() == dev.lens.tolist(), f"{what}: decode"
    assert dec[: len(dev.host)].cpu().numpy().tobytes() == dev.host.tobytes(), f"{what}: the decoded bytes are not the input"
    return got_route


# (route, forced kind, max_len, htable), block 1 MiB: test_gpu_k1_hints.py's C1 / C3 tables
ROUTES = [
    ("s:lean g16 fw40", "", 4096, 1024),
    ("s:lean g8 fw40", "", 8192, 1024),
    ("s:lean g8 fw24", "", 65536, 1024),
    ("s:parse t32", "S", 4096, 1024),
    ("l", "l", 65537, 1024),
    ("l:k1c", "", 65537, 1024),
    ("x", "x", 128 * KiB, 1024),
    ("w:pl", "w", 4096, 1024),
    ("w:win", "w", 20000, 1024),
    ("w:view", "", 0, 1024),
    ("w:pl+gtab", "", 4096, 8192),
]


ROUTE_IDS = [r[0].replace(" ", "-") for r in ROUTES]
every_route = pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)  # the route is in the test's id


def on_route(cuda, what, named, route):
    """The batch on one of ROUTES, which must be the route taken.  (run_route and oracle_bytes
    stand in for test_gpu_k1_hints.py's run_k1 and oracle_of, which fix the block at 1 MiB and
    the slots at ez_compress_bound: here the block varies and the slots are exact.)"""
    name, kind, max_len, htable = route
    assert not max_len or max(len(b) for _, b in named) <= max_len
    assert run_route(cuda, what, named, MiB, htable, kind, max_len, name) == name


def named(cases):
    return [(c.name, c.data) for c in cases]


# ------------------------------------------------------------------ A - G: every route


@pytest.mark.gpu
@every_route
@pytest.mark.parametrize("g", ["A", "B", "C", "E", "G"])
def test_k1_edges_on_every_route(cuda, g, route):
    """Forward counts (A), backward counts (B), window mechanics (C), runs and zeros (E) and the
    token writer's widths (G): the group's cases as one batch on each of the eleven routes."""
    on_route(cuda, f"group {g}", named(ki.group(g)), route)


GLONG_ROUTES = [r for r in ROUTES if r[0] in ("s:lean g8 fw24", "l", "l:k1c", "x", "w:win", "w:view")]


@pytest.mark.gpu
@pytest.mark.parametrize("route", GLONG_ROUTES, ids=[r[0].replace(" ", "-") for r in GLONG_ROUTES])
def test_k1_edges_long_records_and_kemitin(cuda, route):
    """G's cases over 4,096 bytes (4,097 bytes; 2,046..2,049 records) on the six routes that take them."""
    on_route(cuda, "group G (long)", named(ki.group("Glong")), route)


@pytest.mark.gpu
@every_route
def test_k1_edges_position_0_and_before(cuda, route):
    """D: a candidate at position 0 in the pending literal and in the block.  Each case stands
    twice in the batch, after a stream that ends in filler and after one that ends in the very
    8 bytes in front of the case's copy: a kernel that reads before its stream's first byte
    finds more (or, where Go finds the block's zeros there, less) than Go."""
    rng = np.random.default_rng(5)
    batch = []
    for c in ki.group("D"):
        batch.append((f"filler before {c.name}", rng.integers(1, 256, 24, dtype=np.uint8).tobytes()))
        batch.append((c.name, c.data))
        batch.append((f"lure before {c.name}", rng.integers(1, 256, 9, dtype=np.uint8).tobytes() + ki.before_of(c)))
        batch.append((c.name + " after its lure", c.data))
    on_route(cuda, "group D", batch, route)


F_SUBSET = (
    ("A", "A-lane0-len6"), ("A", "A-lane7-len41"), ("A", "A-lane16-len169"), ("B", "B-back9"), ("B", "B-back8-done-after3"),
    ("C", "C-restore-k3"), ("C", "C-evict3-lane0"), ("C", "C-end-len6-window"), ("C", "C-tiny9"), ("D", "D-head-after-3-zeros"),
    ("D", "D-head-len6"), ("D", "D-candidate-7-after-1-zeros"), ("E", "E-zeros9-end"), ("E", "E-period3-run6"), ("E", "E-empty-literal"),
)


def _subset():
    by = {c.name: c for g in "ABCDE" for c in ki.group(g)}
    return [by[n] for _, n in F_SUBSET]


@pytest.mark.gpu
@every_route
def test_k1_edges_placement(cuda, route):
    """F: copies that start at stream positions 55..90, 119..140 and n - 70..n - 60 (the 128-byte
    regions' reloads); a subset of A - E at every stream address mod 4, with streams of 1, 2 and
    3 bytes in front."""
    on_route(cuda, "group F (positions)", named(ki.group("F")), route)
    batch, at = [], 0
    for r in (1, 2, 3, 0):
        for c in _subset():
            pad = (r - at) % 4
            if pad:
                batch.append((f"{pad} bytes", bytes([65 + pad] * pad)))
                at += pad
            batch.append((f"{c.name} at address {r} mod 4", c.data))
            at += len(c.data)
    assert {len(b) for _, b in batch} >= {1, 2, 3}
    on_route(cuda, "group F (address mod 4)", batch, route)


@pytest.mark.gpu
@every_route
def test_k1_edges_first_and_last_stream(cuda, route):
    """F: the subset again, each case as the batch's first and as its last stream (k1_lean's
    edge slots at the batch's first and last 64 bytes), seven filler streams between: 15 small
    batches per route."""
    rng = np.random.default_rng(7)
    mid = [(f"filler {k}", rng.integers(1, 256, int(n), dtype=np.uint8).tobytes()) for k, n in enumerate((70, 5, 300, 64, 1, 129, 2000))]
    for c in _subset():
        on_route(cuda, f"{c.name} first and last", [(c.name + " first", c.data)] + mid + [(c.name + " last", c.data)], route)


# ------------------------------------------------------------------ H: ring semantics


# (forced kind, max_len) -> the route taken with blocks of 1,024 and 4,096 bytes (the automatic
# choice, kind '', as recorded on the device: the general kernel)
RING_ROUTES = [("l", 16384, "l"), ("x", 16384, "x"), ("w", 16384, "w:pl"), ("w", 20000, "w:win"), ("", 16384, "w:pl"), ("", 0, "w:view")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,max_len,route", RING_ROUTES, ids=[f"{k or 'auto'}-{m}-{r}" for k, m, r in RING_ROUTES])
@pytest.mark.parametrize("bs", [1024, 4096])
def test_k1_edges_ring(cuda, bs, kind, max_len, route):
    """H: blocks of 1,024 and 4,096 bytes, streams of 3 to 9 KiB -- trim 1 at distances bs - 40 ..
    bs + 1 with 0, 1 and 30 bytes pending, the far skip (and that it updates the table), the cut
    at bs - 8.  K1L, K1x and the general kernel forced, and the automatic choice."""
    cases = ki.group(f"H{bs}")
    run_route(cuda, f"group H block {bs}", named(cases), bs, cases[0].htable, kind, max_len, route)


# ------------------------------------------------------------------ I, J: K1c and K1x


# (route, forced kind, max_len; None: the batch's longest stream)
LONG_ROUTES = [("l", "l", None), ("l:k1c", "", None), ("x", "x", None), ("x", "", (1 << 19) + 1), ("w:win", "w", None), ("w:view", "", 0)]
long_route = pytest.mark.parametrize("route,kind,max_len", LONG_ROUTES, ids=["l", "l:k1c", "x-forced", "x-auto", "w:win", "w:view"])


def on_long_route(cuda, what, cases, route, kind, max_len):
    longest = max(len(c.data) for c in cases)
    run_route(cuda, what, named(cases), MiB, cases[0].htable, kind, longest if max_len is None else max_len, route)


@pytest.mark.gpu
@long_route
def test_k1_edges_k1c_streams_on_long_routes(cuda, route, kind, max_len):
    """I: streams of 72 .. 100 KiB, sparse events, and one thing at chunk 1's start C = 32,768
    (kc_geom), its warm-up W = 8,192 or its overlap O = 1,024: exact on K1L, K1c, K1x and the
    general kernel (one batch per table size)."""
    for ht in (1024, 4096):
        on_long_route(cuda, f"group I htable {ht}", [c for c in ki.group("I") if c.htable == ht], route, kind, max_len)


@pytest.mark.gpu
def test_k1_edges_k1c_chunk_boundary(cuda):
    """I: each stream alone on K1c with its verdict counted: every stream is either proven by
    K1c or handed to K1L as K1C_VERDICTS says, and exact either way."""
    import eazy_amd as ez

    cases = ki.group("I")
    verdicts = {}
    for c in cases:
        ez.k1c_stats(True)
        try:
            run_route(cuda, c.name, [(c.name, c.data)], MiB, c.htable, "", len(c.data), "l:k1c")
        finally:
            st = ez.k1c_stats(False)
        verdicts[c.name] = [k for k in ("proven", "chunk", "sync", "judge", "cap") if st[k]]
        print(f"K1c verdict: {c.name}: {st}")
        assert sum(st[k] for k in ("proven", "chunk", "sync", "judge", "cap")) == 1, (c.name, st)
    assert verdicts == {"I-" + k: v for k, v in K1C_VERDICTS.items()}, verdicts


# Read from ez_k1_chunk.hip and ez_k1_long.h (kc_parse, long_loop's `keep`, kc_stitch_seq; the first pass
# starts from zero tables: a chunk starts W before its start b with a zero table).  Chunk 0's
# parse is Go's and runs its windows while i < b1 + O (ev.stop), b1 = C; chunk 1 keeps the records
# that end at or after b1; the stream is stitched at the first copy end >= b1 that both have, and
# fails with "sync" when there is none.  Every later chunk start of these streams has a copy end
# 312 bytes past it, so chunk 1's start alone decides.
K1C_VERDICTS = {
    "copy-ends-at-C": ["proven"],  # kept by chunk 1 (end >= b1), shared at C itself
    "copy-starts-at-C": ["proven"],  # shared end C + 12
    "copy-spans-C": ["proven"],  # shared end C + 6
    "zeros-span-C": ["proven"],  # the zero token's end C + 20
    "run-spans-C": ["proven"],  # the run's end C + 20
    # chunk 1's zero table at C - W has no entry for the source, so it has no copy at C + 100;
    # chunk 0 has (it is Go's); both have the next one (ends C + 512), the path switches there
    "source-beyond-warmup": ["proven"],
    "source-within-warmup": ["proven"],  # chunk 1 visits the source in its warm-up and finds the copy itself
    "no-copy-end-in-overlap": ["sync"],  # nothing to stitch at: K1L
    "copy-ends-at-C+O-1": ["proven"],
    "copy-ends-at-C+O+1": ["proven"],  # it starts before C + O: ev.stop bounds the windows' starts, not the copies' ends
    "copy-starts-at-C+O-1": ["proven"],  # the last position a window of chunk 0 is sure to reach
    "copy-starts-at-C+O+15": ["sync"],  # the first position no window of chunk 0 can reach (16 lanes from i < C + O)
}


@pytest.mark.gpu
@long_route
def test_k1_edges_k1x_rounds(cuda, route, kind, max_len):
    """J: streams of 40 .. 80 KiB with 0, 1, 7, 8, 9 and 20 events (K1x's 8 rounds end and the
    rest is handed over), events at positions 16,383 .. 16,385 (its chunk: the event at 16,384 has
    its candidate in the chunk before), a copy whose nearest same-hash predecessor is 16,383,
    16,382 positions back in its chunk and 16,384 back in the chunk before (kx_pred's u16
    distance), a source at the round's start, and events 100, 255, 256 and 257 bytes apart three
    times in a row (kDenseGap's hand-over).  K1x forced and chosen (max_len above 2^19), and the
    other long routes."""
    on_long_route(cuda, "group J", ki.group("J"), route, kind, max_len)
