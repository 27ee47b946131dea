"""Every route exact on dirty scratch: the caller's workspace and the scratch the library keeps
between calls (ez_cache.h's entries, the Readers' shared K2j workspace, the multi-device pool) in four
states when the call starts (tests/dirty.py):

  zero   ez.fill_cached(0x00), workspace zeros: the control (a route that passes this alone needs zeros);
  stale  what a decoy call of the same geometry left, no fill between;
  a5     ez.fill_cached(0xA5), workspace 0xA5;
  ff     ez.fill_cached(0xFF), workspace 0xFF.

Nothing new is built but the decoys: the inputs are the hand-built groups of the route's own tests and
the checks are those tests' runners, so the bar is theirs everywhere: bytes, sizes and statuses equal
to the oracle, guards and sentinels intact, inputs unchanged.  dirty.under() holds what keeps a case
from passing vacuously: one warm call first, the fill covers more than 0 bytes where the route keeps
scratch, and ez.fill_cached(-1) reports the same total before and after the target (it ran in the
dirtied buffers, not in fresh ones).  A K1 decoy is synth.logs bytes cut at the target's own offsets
(plus, on the long routes, one with every stream at max_len); a K2 decoy is a batch of the same count
of T6's nine-literal stream and R6's damaged streams, which must leave longer hand-over and
deferred-literal lists than the target writes (the first test proves the streams are that, on the CPU).

The GPU tests are marked one by one: the first two tests run on the CPU."""

import functools

import numpy as np
import pytest

import dirty
import k1_inputs as ki
import k2r_streams as k2r
import k2t_streams as k2t
import pyoracle as po
from dirty import STATES, under
from k2_streams import HDR, SMALL_MAX, _need, _oracle, _run, _slot

every_state = pytest.mark.parametrize("state", STATES)
MiB, KiB = 1 << 20, 1 << 10


# ------------------------------------------------------------------ K2: targets and decoys (host)


def long_literals(b, least=k2t.DEFER_MIN):
    """Literals of at least `least` bytes on the stream's token chain, up to its first error."""
    n, i = 0, 0
    while i < len(b):
        tag, l, j, err = po.dec_tag(b, i)
        if err:
            break
        if tag == po.META and l == 0:
            _, ml, j, err = po.dec_meta(b, j)
            if err:
                break
            i = j + ml
        elif tag == po.LITERAL:
            n += l >= least
            i = j + l
        else:
            _, j, err = po.dec_offset(b, j, l)
            if err:
                break
            i = j
    return n


def _r_target(cases):
    """test_gpu_k2r._go's arguments for a group of Case(name, stream, slot)."""
    slots = {s: c.slot if c.slot is not None else 17 + s % 5 for s, c in enumerate(cases) if c.slot is not None or _need(c.stream) < 15}
    handed = k2r.expected_handed([c._replace(slot=slots.get(s)) for s, c in enumerate(cases)])
    return dict(ins=[c.stream for c in cases], slots=slots, handed=handed, kind="r", max_len=True)


def _t_target(named, given, kind):
    """test_gpu_k2t._rings' batch A (the 8 KiB ring): the group and one stream with a slot over 4 KiB."""
    from k2_streams import lit, rb
    from test_gpu_k2t import _slots

    ins = [b for _, b in named] + [HDR + lit(rb(np.random.default_rng(2199), 5000))]
    return dict(ins=ins, slots=_slots(ins, given), handed="auto", kind=kind, max_len=True)


def _t7():
    named, slots = [], {}
    for name, b, need in k2t.t7_streams():
        for d in (0, 1):
            slots[len(named)] = need - d
            named.append((f"{name}-{d}", b))
    return named, slots


K2_TARGETS = ("K2r-R4-pairs", "K2r-R5-slot-edges", "K2r-R6-mixed-wave", "K2t-T6-deferred", "K2t-T7-slots", "K2w-T6-deferred",
              "K2j-copies-handed", "K2j-phase-never-merges", "K2j-short-slot-handed")


@functools.lru_cache(maxsize=None)
def k2_targets():
    """{name: _run's arguments}: the groups that hand streams over, defer literals or never merge."""
    import test_gpu_k2j as kj

    g = {}
    g["K2r-R4-pairs"] = _r_target(k2r.r4_streams())
    g["K2r-R5-slot-edges"] = _r_target(k2r.r5_streams())
    g["K2r-R6-mixed-wave"] = _r_target(k2r.r6_streams())
    g["K2t-T6-deferred"] = _t_target(k2t.t6_streams(), {}, "t")
    g["K2t-T7-slots"] = _t_target(*_t7(), "t")
    g["K2w-T6-deferred"] = _t_target(k2t.t6_streams(), {}, "w")
    g["K2j-copies-handed"] = dict(ins=[b for _, b in kj.copy_streams()], slots=None, handed={3}, kind="j")
    g["K2j-phase-never-merges"] = dict(ins=[kj.phase_stream(f, 40000)[0] for f in (12, 13)], slots=None, handed=set(), kind="j")
    rng = np.random.default_rng(303)
    three = [HDR + kj.lit(kj.rb(rng, 300)) + kj.cpy(200, 150) + kj.cpy(1, 70) for _ in range(3)]
    g["K2j-short-slot-handed"] = dict(ins=three, slots={1: _need(three[1]) - 1}, handed={1}, kind="j")
    assert tuple(g) == K2_TARGETS
    return g


@functools.lru_cache(maxsize=None)
def _decoy_parts():
    nine = dict(k2t.t6_streams())["t6-nine-long-literals"]
    damaged = [c.stream for c in k2r.r6_streams() if ("truncated" in c.name or "bit-flip" in c.name) and _oracle(c.stream, 1 << 20)[1] != 0]
    good = [c.stream for c in k2r.r6_streams() if c.name.endswith("good")]
    assert len(damaged) >= 30 and long_literals(nine) == 9
    return nine, damaged, good


def k2_decoy(count, kind):
    """A batch of `count` streams that hands over and defers more than any target of that count: every
    second stream, and the last, damaged (R6's truncated and bit-flipped streams the oracle refuses; never
    stream 0, so that a stale list entry is a non-zero word), the others T6's stream of nine literals of
    16 KiB and more where the decoder defers (K2t, K2w), else a good R6 stream."""
    nine, damaged, good = _decoy_parts()
    clean = [nine] if kind in ("t", "w") else good
    bad = lambda s: s % 2 == 1 or (s == count - 1 and s > 0)  # noqa: E731
    return [damaged[(s // 2) % len(damaged)] if bad(s) else clean[(s // 2) % len(clean)] for s in range(count)]


def _bad(ins, slots):
    """Streams the oracle gives an error, or whose output does not fit their slot."""
    n = 0
    for s, b in enumerate(ins):
        cap = slots[s] if slots and s in slots else _slot(s, _need(b))
        n += cap < 16 or _oracle(b, cap)[1] != 0
    return n


@pytest.mark.parametrize("name", K2_TARGETS)
def test_k2_decoys_are_what_they_claim(name):
    """CPU.  By the oracle, the decoy of every K2 target has more erroring or too-small streams than
    the target, and, where the decoder defers literals, more literals of at least 16,384 bytes."""
    t = k2_targets()[name]
    d = k2_decoy(len(t["ins"]), t["kind"])
    assert len(d) == len(t["ins"])
    assert _bad(d, None) > _bad(t["ins"], t["slots"]), (name, _bad(d, None), _bad(t["ins"], t["slots"]))
    if t["kind"] in ("t", "w"):
        want, have = sum(long_literals(b) for b in t["ins"]), sum(long_literals(b) for b in d)
        assert have > want and (want > 0) == ("T6" in name), (name, have, want)


def test_fill_cached_needs_a_device():
    """CPU.  ez.fill_cached raises DeviceError without a device, as the other compute wrappers do;
    with one, counting touches nothing and a byte outside 0..255 is refused."""
    import eazy_amd as ez

    if ez.device_count() <= 0:
        with pytest.raises(ez.DeviceError):
            ez.fill_cached(0x00)
        with pytest.raises(ez.DeviceError):
            ez.fill_cached(-1)
        return
    assert ez.fill_cached(-1) == ez.fill_cached(-1)
    for byte in (256, -2):
        with pytest.raises(ez.Panic):
            ez.fill_cached(byte)


@pytest.mark.gpu
def test_fill_cached_writes_what_it_counts(cuda, reset_batch):
    """The hook itself, seen through the two introspection calls that read the library's scratch
    back: after fill_cached(b) ez_segments_last's hand-over count (a uint64 of segs_cache's entry) is
    eight bytes of b and ez_decompressed_size_parts_last's counters (uint32s of size_cache's entry)
    four; counting changes nothing; release_cached leaves nothing to count."""
    import torch

    import eazy_amd as ez
    import test_gpu_k2z_parts as p
    import test_gpu_segments as g

    ez.release_cached()
    assert ez.fill_cached(-1) == 0 and ez.fill_cached(0x11) == 0
    ins = reset_batch[0][:4]
    comp, d_coff, d_ooff, _, _ = g._inputs(cuda, ins, [len(t) for t in reset_batch[1][:4]])
    ez.decompress_batch_segmented(comp, d_coff, d_ooff)
    torch.cuda.synchronize()
    assert ez.segments_last() == (16, 0, 0)
    segs = ez.fill_cached(-1)
    assert segs > 0 and ez.segments_last() == (16, 0, 0)
    whole, pc, pcoff, nin = p._upload(cuda, [p._long(40000, 331)])
    ez.select_size_route("p")
    try:
        ez.decompressed_sizes(pc, pcoff, max_len=p.HINT[256], in_bytes=nin)
        torch.cuda.synchronize()
        parts = ez.decompressed_size_parts_last()
    finally:
        ez.select_size_route("")
    both = ez.fill_cached(-1)
    assert parts[0] == 3 and both > segs
    for byte in (0xA5, 0xFF, 0x00):
        assert ez.fill_cached(byte) == both
        assert ez.segments_last()[1] == int.from_bytes(bytes([byte]) * 8, "little")
        assert ez.decompressed_size_parts_last() == (int.from_bytes(bytes([byte]) * 4, "little"),) * 3
    assert ez.fill_cached(0x5A, device=0) == both and ez.fill_cached(-1) == both
    ez.release_cached()
    assert ez.fill_cached(-1) == 0


# ------------------------------------------------------------------ K2: batch decode with ez_decompress_workspace


def _jc(ins):
    return 256 if sum(len(b) for b in ins) <= SMALL_MAX else 1024


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("name", K2_TARGETS)
def test_k2_batch_decode(cuda, name, state):
    """K2r on R4, R5 and R6, K2t on T6 and T7, K2w on T6, K2j on the groups that hand over or never
    merge; the exact decoder alone runs behind each on the same dirt (k2_streams._run).  K2j's
    workspace is the library's (jump_cache): there the fill must cover it."""
    t = k2_targets()[name]
    kind, count = t["kind"], len(t["ins"])

    def go(ins, slots, handed, ws_init):
        return _run(cuda, ins, _jc(ins) if kind == "j" else None, slots=slots, handed=handed, kind=kind, max_len=t.get("max_len"), pad=0, ws_init=ws_init)

    def decoy(first):
        _, handed, deferred = first
        left, _, _ = go(k2_decoy(count, kind), None, "auto", 0)
        dirty.assert_decoy_left_more(left, count, handed, deferred, kind in ("t", "w"))
        return left

    under(state, lambda ws_init: go(t["ins"], t["slots"], t["handed"], ws_init), decoy, scratch=kind == "j", what=name)


# ------------------------------------------------------------------ K1: batch compress


def _log_batch(cuda, offs, seed):
    """synth.logs bytes cut at the offsets `offs`, on the device."""
    import torch

    from eazy_amd import synth

    host = synth.logs(seed, max(int(offs[-1]), 1))[: int(offs[-1])]
    return torch.from_numpy(host.copy()).to(cuda), torch.from_numpy(np.asarray(offs, np.int64)).to(cuda)


def k1_decoys(cuda, lens, block, htable, kind, max_len, route, full):
    """The decoy calls of a K1 target: the same count, max_len, block, table and forced kind on log
    bytes cut at the target's own offsets, and (full) once more with every stream at max_len.  Each
    must take the target's route and leave the cached scratch at its size."""
    import torch

    import eazy_amd as ez

    before = ez.fill_cached(-1)
    longest = max_len if max_len else max(lens)
    batches = [np.concatenate([[0], np.cumsum(lens)])]
    if full:
        batches.append(np.arange(len(lens) + 1, dtype=np.int64) * longest)
    for k, offs in enumerate(batches):
        data, off = _log_batch(cuda, offs, 70 + k)
        ez.select_compress_kernel(kind)
        try:
            cb = ez.compress_batch(data, off, block, htable, max_len=max_len)
            torch.cuda.synchronize()
            took = ez.compress_route_last()
        finally:
            ez.select_compress_kernel("")
        assert took == route, f"the decoy took {took!r}, the target {route!r}"
        assert int(cb.status.abs().sum()) == 0
    assert ez.fill_cached(-1) == before, "the decoy did not run in the target's scratch"


NO_SCRATCH = ("w:pl", "w:win", "w:view")  # the general kernel with its table in LDS keeps nothing


def k1_under(cuda, state, what, named, block, htable, kind, max_len, route, full=False):
    from test_gpu_k1_edges import run_route

    lens = [len(b) for _, b in named]

    def target(_):
        assert run_route(cuda, what, named, block, htable, kind, max_len, route) == route

    under(state, target, lambda _: k1_decoys(cuda, lens, block, htable, kind, max_len, route, full), scratch=route not in NO_SCRATCH,
          what=f"{what} on {route}")


def _edges():
    import test_gpu_k1_edges as e

    return e


def _route_ids(routes):
    return [r[0].replace(" ", "-") for r in routes]


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("route", _edges().ROUTES, ids=_route_ids(_edges().ROUTES))
def test_k1_every_route(cuda, route, state):
    """Window mechanics (C), runs and zeros (E) and the token writer's widths (G), one batch each, on
    the eleven routes: k1_lean's records and edge area, k1_parse's records, K1L's and K1x's scratch,
    K1c's ten regions (short streams: one chunk each), the general kernel's global tables."""
    name, kind, max_len, htable = route
    for g in ("C", "E", "G"):
        k1_under(cuda, state, f"group {g}", _edges().named(ki.group(g)), MiB, htable, kind, max_len, name)


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("route", _edges().GLONG_ROUTES, ids=_route_ids(_edges().GLONG_ROUTES))
def test_k1_long_records(cuda, route, state):
    """G's cases of 4,097 bytes (2,046 .. 2,049 records each) on the six routes that take them."""
    name, kind, max_len, htable = route
    k1_under(cuda, state, "group G (long)", _edges().named(ki.group("Glong")), MiB, htable, kind, max_len, name)


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("route,kind,max_len", _edges().LONG_ROUTES, ids=["l", "l:k1c", "x-forced", "x-auto", "w:win", "w:view"])
def test_k1_long_routes(cuda, route, kind, max_len, state):
    """I (72 .. 100 KiB, table 1,024 and 4,096) and J (40 .. 80 KiB): ragged batches on K1L, K1c (its
    chunk slots past a short stream's end hold the all-max_len decoy's chunks), K1x and the general
    kernel."""
    groups = [("I htable 1024", [c for c in ki.group("I") if c.htable == 1024]), ("I htable 4096", [c for c in ki.group("I") if c.htable == 4096]),
              ("J", ki.group("J"))]
    for what, cases in groups:
        longest = max(len(c.data) for c in cases)
        k1_under(cuda, state, f"group {what}", _edges().named(cases), MiB, cases[0].htable, kind, longest if max_len is None else max_len, route,
                 full=True)


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("kind,max_len,route", _edges().RING_ROUTES, ids=[f"{k or 'auto'}-{m}-{r}" for k, m, r in _edges().RING_ROUTES])
def test_k1_ring(cuda, kind, max_len, route, state):
    """H at a block of 1,024 bytes: the ring's trims and the far skip on K1L, K1x and the general kernel."""
    cases = ki.group("H1024")
    k1_under(cuda, state, "group H block 1024", _edges().named(cases), 1024, cases[0].htable, kind, max_len, route, full=route in ("l", "x"))


@pytest.mark.gpu
@every_state
def test_k1_global_tables_serve_several_streams(cuda, state):
    """2,100 tiny streams at a table of 8,192 entries: the general kernel's grid is 2,048 blocks, so
    a block's table in global scratch serves a second stream after its first."""
    cases = [c for g in ("C", "E") for c in ki.group(g)]
    named = [(f"{cases[s % len(cases)].name} (copy {s // len(cases)})", cases[s % len(cases)].data) for s in range(2100)]
    k1_under(cuda, state, "2,100 tiny streams", named, MiB, 8192, "", 4096, "w:pl+gtab")


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("kind,htable,route", [("", 1024, "s:parse t16 mw"), ("", 8192, "w:view+gtab")], ids=["split", "general"])
def test_k1_multi_write(cuda, kind, htable, route, state):
    """The small multi-Write cases at block 65,536 on the split route (split_scratch_words with
    write_idx) and on the general kernel's multi-Write variant with its tables in global scratch."""
    import torch

    import eazy_amd as ez
    import test_gpu_k1_writes as w
    from eazy_amd import synth

    (block, _), cases = w.main_config()
    named = w.named(cases)

    def target(_):
        w.run_writes(cuda, "the small cases", named, block, htable, kind, route)

    def decoy(_):
        before = ez.fill_cached(-1)
        logs, at, fake = synth.logs(75, sum(len(p) for _, ws in named for p in ws) + 1).tobytes(), 0, []
        for name, ws in named:
            fake.append((name, tuple(logs[at + sum(len(q) for q in ws[:k]) : at + sum(len(q) for q in ws[: k + 1])] for k in range(len(ws)))))
            at += sum(len(p) for p in ws)
        wb = w.WriteBatch(cuda, fake)
        caps = [int(ez.compress_bound(int(n))) + 5 * len(ws) + 16 for n, (_, ws) in zip(wb.lens, fake)]
        took, st, *_ = wb.compress(block, htable, kind, caps)
        assert took == route and not st.any()
        assert ez.fill_cached(-1) == before, "the decoy did not run in the target's scratch"

    under(state, target, decoy, what=f"multi-Write on {route}")


# ------------------------------------------------------------------ K3


@pytest.mark.gpu
@pytest.mark.parametrize("more,fewer", [(2049, 1025), (2049, 1), (262145, 2049)])
def test_k3_pack_on_a_larger_packs_workspace(cuda, more, fewer):
    """K3 runs on a filled workspace in its own tests; here on the workspace a pack of more streams
    left (its tile sums past the smaller batch's tiles and in them)."""
    import test_gpu_k3_pack as k3

    left = k3.run_pack(cuda, k3.p3_batch(more), src_shift=1, dst_shift=2)
    assert left.numel() > 8 * ((fewer + 1023) // 1024) and left.cpu().numpy().any()
    k3.run_pack(cuda, k3.p3_batch(fewer), src_shift=fewer & 3, dst_shift=3, ws_init=left)


# ------------------------------------------------------------------ K2z, its parts route, K2g


def _all_refused(ins):
    """The decoy of a size query or a segment query: the same count, every stream with a literal cut
    short at its end (every stream handed over, the long ones still walked chunk by chunk)."""
    return [(b if b else HDR) + b"\x03ab" for b in reversed(ins)]


@pytest.mark.gpu
@every_state
@pytest.mark.parametrize("route", ["lane", "wave"])
def test_k2z_size_query(cuda, route, state):
    """The lane kernel on 4,096 short streams and the wave kernel at every chunk size on streams with
    errors, a MetaReset after output (handed over by design) and a 70,000-byte literal: the first list,
    K2g's counters and the second list in the workspace's spare words start dirty."""
    import test_gpu_k2z as z

    rng = np.random.default_rng(239)
    small = z._small_streams()
    late = HDR + z.lit(b"a") + z.meta(z.META_RESET, b"\x14") + z.lit(b"b")
    if route == "lane":
        special = {7: b"", 64: HDR, 100: HDR + b"\x03ab", 1000: late, 4095: HDR + z.lit(z.rb(rng, 3000)) + z._tail3()}
        ins, design = [special.get(s, small[s % len(small)]) for s in range(4096)], (1000,)
        kw = dict(hints=(4096,), route={4096: 1})
    else:
        ins = small[:20] + [b"", HDR, HDR + b"\x03ab", z.fill_to(HDR, 64 * 256 + 40, rng), HDR + z.lit(z.rb(rng, 70000)) + z._tail3(), late,
                            z.fill_to(HDR, 5000, rng)] + small[20:40]
        design, kw = (25,), dict(hints=(4096, 4097, 1 << 20))

    def decoy(_):
        keep = []
        z._run_size(cuda, _all_refused(ins), keep=keep, **kw)
        w = keep[-1].cpu().numpy().view(np.uint32)
        assert int(w[0]) == len(ins) and w[1 : len(ins) + 1].any()
        return keep[-1]

    under(state, lambda ws_init: z._run_size(cuda, ins, design=design, ws_init=ws_init, **kw), decoy, scratch=False, what=f"K2z {route}")


@pytest.mark.gpu
@every_state
def test_k2z_parts_route(cuda, state):
    """The parts route (size_cache: the header words, the part counts' scan, the records) on 65 mixed
    streams (errors, hand-overs by design, long streams cut inside a token) and on the adversarial
    literals whose parts are walked again."""
    import test_gpu_k2z_parts as p

    ins, design = p._mixed(65, np.random.default_rng(341))
    want = p._want(ins)
    design = [s for s in design if want[s][1] == 0]
    adv = []
    for parts in (2, 3):  # (test_adversarial_and_garbage's first two streams)
        b = HDR + b"\x00"
        while len(b) < parts * 64 * 256 + 700:
            b += p.lit(b"\x10\x85" * 128)
        adv.append(b + p._tail3())

    def target(ws_init):
        got = p._run_parts(cuda, ins, design=design, chunks=(256,), ws_init=ws_init)
        assert got[256][1] > 0
        again = p._run_parts(cuda, adv, chunks=(256,), ws_init=ws_init)
        assert again[256][2] > 0, again

    def decoy(_):
        keep = []
        p._run_parts(cuda, _all_refused(ins), chunks=(256,), keep=keep)
        assert int(keep[-1][:4].cpu().numpy().view(np.uint32)[0]) == len(ins)
        return keep[-1]

    under(state, target, decoy, what="K2z parts")


from test_gpu_segments import dumped, reset_batch  # noqa: E402,F401  (fixtures)


def _mixed_segments(dumped, reset_batch):
    """test_gpu_segments.py's mixed batch: valid 4-segment streams, an error in segment 2 of 4 (three
    kinds), plain streams and empty ones."""
    from k2_streams import cpy, lit, rb

    rng = np.random.default_rng(9)
    valid = reset_batch[0][:5]
    damaged = [e[2] for e in dumped if " in segment 2 of 4" in e[0] and e[1] == 0]
    plain = [HDR + lit(rb(rng, 3000)) + cpy(500, 2000), HDR + lit(rb(rng, 70)), HDR]
    assert len(damaged) == 3
    return valid[:2] + damaged + plain[:1] + [b""] + valid[2:] + plain[1:] + [b""]


@pytest.mark.gpu
@every_state
def test_k2g_segmented_decode(cuda, dumped, reset_batch, state):
    """ez_decompress_batch_segmented (segs_cache: the hints, the segment arrays, the query's and the
    decode's workspaces, the segments' sizes and statuses) on streams with cuts and with an error in
    segment 2 of 4, against the exact decoder and the oracle."""
    import eazy_amd as ez
    import test_gpu_segments as g

    ins = _mixed_segments(dumped, reset_batch)
    caps = [_slot(s, _need(b)) for s, b in enumerate(ins)]

    def target(_):
        _, st, took = g._decode_both(cuda, ins, caps)
        assert took == "r" and sorted(np.flatnonzero(st != 0)) == [2, 3, 4]
        segs = ez.segments_last()
        assert segs[0] == 5 * 4 + 3 * 3 + 3 + 2 and segs[1] >= 3

    def decoy(_):
        other = list(reversed(ins))
        g._decode_both(cuda, other, [_slot(s, _need(b)) for s, b in enumerate(other)])

    under(state, target, decoy, what="segmented decode")


@pytest.mark.gpu
@every_state
def test_k2g_segment_query(cuda, dumped, state):
    """ez_stream_segments_batch on the host check's streams with cuts (up to 40 in a stream: the kept
    cuts and the fill pass) and with an error in segment 2 of 4: the workspace's header word and kept
    cuts start dirty, the arrays must equal the host walk's."""
    import test_gpu_segments as g

    sel = [e for e in dumped if e[1] == 0 and (len(e[3]) >= 3 or " in segment 2 of 4" in e[0])]
    first = [max(sel, key=lambda e: len(e[3]))] + [e for e in sel if " in segment 2 of 4" in e[0]]
    group = first + [e for e in sel if not any(e is f for f in first)][: 48 - len(first)]
    assert len(group[0][3]) > 16 and len(first) >= 4
    caps = [(e[3][-1][1] if e[3] else 0) + 1 + s % 9 for s, e in enumerate(group)]

    def run(entries, slots, ws_init, keep=None):
        comp, d_coff, d_ooff, coff, ooff = g._inputs(cuda, [e[2] for e in entries], slots)
        idx, sin, sout = g._expected(entries, coff, ooff)
        found = int(idx[-1])
        for cap in (found + 3, len(entries)):  # room for every cut, and the one-segment-per-stream layout
            seg_idx, seg_in, seg_out, total = g._query(cuda, comp, d_coff, d_ooff, len(entries), cap, ws_init=ws_init, keep=keep)
            if cap >= found:
                assert tuple(total) == (found, found) and np.array_equal(seg_idx, idx)
                assert np.array_equal(seg_in[: found + 1], sin) and np.array_equal(seg_out[: found + 1], sout)
            else:
                assert tuple(total) == (len(entries), found) and list(seg_idx) == list(range(len(entries) + 1))
                assert list(seg_in[: len(entries) + 1]) == list(coff) and list(seg_out[: len(entries) + 1]) == list(ooff)

    def decoy(_):
        keep = []
        run(list(reversed(group)), list(reversed(caps)), 0, keep)
        assert keep[0].cpu().numpy()[64:].any()  # (kept cuts of other streams in every stream's place)
        return keep[-1]  # (the one-segment layout's: its header word says so)

    under(state, lambda ws_init: run(group, caps, ws_init), decoy, scratch=False, what="segment query")


@pytest.mark.gpu
@every_state
def test_k2g_sizes_of_concatenated_streams(cuda, dumped, state):
    """decompressed_sizes on concatenated streams: K2z hands them over, K2g's stage sizes them and
    lists the rest again for the exact decoder in the workspace's spare words."""
    import test_gpu_size_segments as q

    group = [(e[0], e[1], e[2], len(e[3]), 0) for e in dumped if e[1] == 0][:80]
    ins = [e[2] for e in group] + [b"", HDR] + q._truncations([(e[0], e[1], e[2], len(e[3]), 0) for e in dumped])[:9]

    def target(ws_init):
        for hint in (4096, 65536):
            sz, st, (taken, sized, handed) = q._query(cuda, ins, 0, hint, ws_init=ws_init)
            assert sized > 20 and handed > 0, (taken, sized, handed)

    def decoy(_):
        keep = []
        q._query(cuda, _all_refused(ins), 0, 65536, keep=keep)
        w = keep[0].cpu().numpy().view(np.uint32)
        n = len(ins)
        assert int(w[0]) == n and int(w[n + 3]) > 0 and w[n + 4 : 2 * n + 4].any()  # both lists longer than the target's
        return keep[0]

    under(state, target, decoy, scratch=False, what="sizes of concatenated streams")


# ------------------------------------------------------------------ scratch behind handles and the host path


@pytest.mark.gpu
@every_state
def test_write_many_staging(cuda, state):
    """ez_writer_write_many (many_cache: the pinned staging, the device buffer, the records) on one
    round of test_gpu_write_many.py's mix on fresh handles, behind one handle that stays: the call
    leases the scratch of its first handle's HIP stream, and that handle's stream goes on from call to
    call, so its bytes are the oracle's for its Writes so far."""
    import test_gpu_write_many as m

    lib = m.Lib()
    try:
        first = lib.new(65536, 1024)
        ls = m.lines(80, 8, 100, 3000)
        written = []

        def call(rows, shared):
            written.append(ls[len(written)])
            want = m.kw.oracle_writes(65536, 1024, written)[-1]
            rc, got, st, _ = lib.many([first] + [r[0] for r in rows], [written[-1]] + [r[1] for r in rows])
            assert rc == 0 and st == [0] * (len(rows) + 1)
            for j, (w, b) in enumerate(zip([want] + [r[2] for r in rows], got)):
                assert b == w, f"handle {j}: {m.first_difference(b, w)}"
            assert lib.counts() == (1 + shared, len(rows) - shared)
            assert lib.ez.compress_route_last() == "hm:lds+own"

        def target(_):
            call(m._mix(lib), 3)

        def decoy(_):  # (six long Writes in the launch and one on its handle's own path: the target's route)
            long = m.lines(79, 7, 30000, 49152)
            rows = [(lib.new(65536, 1024), p, m.kw.oracle_writes(65536, 1024, [p])[0]) for p in long[:6]]
            rows.append((lib.new(65536, 8192), long[6], m.kw.oracle_writes(65536, 8192, [long[6]])[0]))
            call(rows, 6)

        under(state, target, decoy, what="write_many")
    finally:
        lib.ez.select_compress_kernel("")
        lib.free()


@pytest.mark.gpu
@every_state
def test_reader_whole_decode(cuda, state):
    """A NewReaderBytes handle's whole-stream decode of 300,000 log bytes (K2j in the Readers' shared
    workspace); stale: after another handle decoded a longer, different stream."""
    import test_gpu_reader_sized as r
    from eazy_amd import synth

    b = r._stream([synth.logs(95, 300_000).tobytes()])
    longer = r._stream([synth.logs(96, 700_000).tobytes()])
    assert len(b) >= 16384

    def target(_):
        rb, n = r._check(b, 65536)
        assert n == 300_000 and rb.r.whole_decoded and rb.r.whole_launches == 1

    def decoy(_):
        rb, n = r._check(longer, 1 << 20)
        assert n == 700_000 and rb.r.whole_decoded

    under(state, target, decoy, what="Reader whole decode")


@pytest.mark.gpu
@every_state
def test_multi_device_calls(cuda, state):
    """decompressed_sizes_multi and decompress_batch_multi over two shards of device 0 on ragged
    streams with empty and erroring ones: the pooled ws, size, status, in and out buffers are scratch
    too.  Statuses, sizes and the bytes of clean streams equal the single-device results (the bytes
    of a host slot past out_size are unspecified on this path)."""
    import torch

    import eazy_amd as ez
    from test_gpu_size_multi import _ragged

    ins = _ragged()
    off = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
    comp = np.frombuffer(b"".join(ins), np.uint8)
    d_comp, d_off = torch.from_numpy(comp.copy()).to(cuda), torch.from_numpy(off).to(cuda)
    d_sz, d_st = ez.decompressed_sizes(d_comp, d_off)
    ooff = np.concatenate([[0], np.cumsum((d_sz.cpu().numpy() + 15) & ~15)]).astype(np.int64)
    d_out, d_sz2, d_st2 = ez.decompress_batch(d_comp, d_off, torch.from_numpy(ooff).to(cuda))
    torch.cuda.synchronize()
    d_sz, d_st, d_out, d_sz2, d_st2 = (t.cpu().numpy() for t in (d_sz, d_st, d_out, d_sz2, d_st2))
    assert (d_st != 0).sum() >= 2 and (d_st == 0).sum() >= 8

    warmed = []

    def target(_):
        if not warmed:
            # (two shards take the pool's two resources in either order: first a batch of twice the
            # streams, so that both resources and their streams' scratch hold any shard of the target)
            c2, o2 = np.concatenate([comp, comp]), np.concatenate([off, off[1:] + off[-1]])
            sz, _ = ez.decompressed_sizes_multi(c2, o2, devices=[0, 0])
            ez.decompress_batch_multi(c2, o2, np.concatenate([[0], np.cumsum((sz + 15) & ~15)]).astype(np.int64), devices=[0, 0])
            warmed.append(True)
        sz, st = ez.decompressed_sizes_multi(comp, off, devices=[0, 0])
        assert np.array_equal(sz, d_sz) and np.array_equal(st, d_st)
        out, sz, st = ez.decompress_batch_multi(comp, off, ooff, devices=[0, 0])
        assert np.array_equal(sz, d_sz2) and np.array_equal(st, d_st2)
        for s in range(len(ins)):
            if st[s] == 0:
                a = int(ooff[s])
                assert out[a : a + int(sz[s])].tobytes() == d_out[a : a + int(sz[s])].tobytes(), s

    def decoy(_):
        other = _all_refused(ins)
        o2 = np.concatenate([[0], np.cumsum([len(b) for b in other])]).astype(np.int64)
        c2 = np.frombuffer(b"".join(other), np.uint8)
        sz, st = ez.decompressed_sizes_multi(c2, o2, devices=[0, 0])
        assert (st != 0).all()
        ez.decompress_batch_multi(c2, o2, np.concatenate([[0], np.cumsum((sz + 15) & ~15)]).astype(np.int64), devices=[0, 0])

    under(state, target, decoy, what="multi-device calls")
