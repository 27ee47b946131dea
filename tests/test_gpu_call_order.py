"""Call order and concurrency: every route after a different route on the same scratch, two batches in
flight on two HIP streams from one host thread (the shipped schedule), and two host threads with a
stream each (as ez_*_batch_multi runs its shards).

The library's scratch is keyed by (device, stream) and grows only: a route that follows a larger one
runs in the larger one's leftovers, one that follows a smaller one frees and allocates.  The rotation
test runs the K1 batches of tests/test_gpu_dirty_scratch.py in a fixed cyclic order forwards and then
backwards on the default stream (every route after two different predecessors, after a larger and after
a smaller scratch), and the decoders one after another on the contents of one workspace sized for the
largest count, as a caller with one workspace would use it.  The stream tests run three batches whose
automatic routes differ -- P: 300 ragged streams of at most 4 KiB with empty ones (k1_lean, K3, K2r);
Q: four 256 KiB log streams (K1c behind K1L's routing, K3, K2t); R: two log streams of a little over
1 MiB under a max_len hint above 2^19 (K1x, K3, K2j by the automatic rule) -- with every tensor
allocated up front, no synchronisation until the schedule's end, and automatic routing only (the
ez_select_* switches and the *_last introspection are process-wide): the routes are recorded and
asserted in a serial pre-run of the same batches.  The bar is the runners': every compressed stream
equal to the oracle's bytes, every decode equal to the input, statuses 0, guards intact.  One pass
each: none of this is a loop hunting for a race."""

import threading

import numpy as np
import pytest

import dirty
import k1_inputs as ki
from test_gpu_k1_edges import LONG_ROUTES, RING_ROUTES, ROUTES, named, oracle_bytes, run_route
from test_gpu_k1_hints import FILL, GUARD, DevBatch

pytestmark = pytest.mark.gpu
MiB = 1 << 20


# ------------------------------------------------------------------ rotation on one stream


def _k1_rotation():
    """[(route, call(cuda))], the K1 batches of tests/test_gpu_dirty_scratch.py: the eleven routes on
    group C; K1L, K1c and K1x on I's ragged 72 .. 100 KiB streams; K1L and K1x on H's 1,024-byte block;
    G's 4,097-byte streams on k1_lean and K1x; 2,100 tiny streams on the general kernel's global tables;
    the small multi-Write cases on the split route and on the general kernel."""
    import test_gpu_k1_writes as w

    def one(what, batch, block, htable, kind, max_len, route):
        return route, lambda cuda: run_route(cuda, f"{what} on {route}", batch, block, htable, kind, max_len, route)

    out = [one("group C", named(ki.group("C")), MiB, r[3], r[1], r[2], r[0]) for r in ROUTES]
    long = [c for c in ki.group("I") if c.htable == 1024]
    longest = max(len(c.data) for c in long)
    for route, kind, max_len in LONG_ROUTES[:3]:
        out.append(one("group I", named(long), MiB, 1024, kind, longest if max_len is None else max_len, route))
    h = ki.group("H1024")
    for kind, max_len, route in RING_ROUTES[:2]:
        out.append(one("group H", named(h), 1024, h[0].htable, kind, max_len, route))
    for r in (ROUTES[2], ROUTES[6]):
        out.append(one("group G (long)", named(ki.group("Glong")), MiB, r[3], r[1], r[2], r[0]))
    tiny = [c for g in ("C", "E") for c in ki.group(g)]
    out.append(one("2,100 tiny streams", [(f"{tiny[s % len(tiny)].name} (copy {s // len(tiny)})", tiny[s % len(tiny)].data) for s in range(2100)],
                   MiB, 8192, "", 4096, "w:pl+gtab"))
    (block, _), cases = w.main_config()
    for htable, route in ((1024, "s:parse t16 mw"), (8192, "w:view+gtab")):
        out.append((route, lambda cuda, htable=htable, route=route: w.run_writes(cuda, "the small multi-Write cases", w.named(cases), block, htable, "", route)))
    return out


def test_k1_routes_in_rotation(cuda):
    """Twenty-one K1 batches on thirteen routes one after another on the default stream's scratch
    entry, forwards and then backwards, synchronised between calls (run_route, run_writes): every
    call exact."""
    import eazy_amd as ez

    ez.release_cached()
    calls = _k1_rotation()
    assert len(calls) == 21 and len({route for route, _ in calls}) == 13
    sizes = []
    for route, call in calls + calls[::-1]:
        call(cuda)
        sizes.append(ez.fill_cached(-1))
    assert max(sizes) > 0 and sizes == sorted(sizes)  # (grow-only: later calls ran in earlier calls' scratch)
    print(f"K1 rotation: scratch after each call {sizes[: len(calls)]}")


class Shared:
    """The contents of one workspace that every decoder uses in turn (the runners copy it in between
    their guards and hand back what the call left)."""

    def __init__(self, cuda, nbytes):
        import torch

        self.t = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)

    def took(self, left):
        n = min(self.t.numel(), left.numel())
        self.t[:n].copy_(left.reshape(-1)[:n])


from test_gpu_segments import dumped, reset_batch  # noqa: E402,F401  (fixtures)


def test_decoders_in_rotation_on_one_workspace(cuda, dumped, reset_batch):
    """K2r, K2t, K2w, K2j, K2z's lane, wave and parts routes, the segment query and the segmented
    decode, forwards and backwards, each starting on what the call before left in the workspace
    (and in the library's scratch): every call exact."""
    import eazy_amd as ez
    import test_gpu_dirty_scratch as d
    import test_gpu_k2z as z
    import test_gpu_k2z_parts as p
    import test_gpu_segments as g
    from k2_streams import HDR, _need, _run, _slot

    L = ez._lib()
    sh = Shared(cuda, max(L.ez_decompress_workspace(4096), L.ez_segments_workspace(4096)))
    small = z._small_streams()
    late = HDR + z.lit(b"a") + z.meta(z.META_RESET, b"\x14") + z.lit(b"b")
    lane = [late if s == 1000 else (HDR + b"\x03ab" if s == 100 else small[s % len(small)]) for s in range(4096)]
    wave = small[:20] + [b"", HDR, HDR + b"\x03ab", late, z.fill_to(HDR, 64 * 256 + 40, np.random.default_rng(239))] + small[20:40]
    mixed, design = p._mixed(65, np.random.default_rng(341))
    want = p._want(mixed)
    design = [s for s in design if want[s][1] == 0]
    segs = d._mixed_segments(dumped, reset_batch)
    caps = [_slot(s, _need(b)) for s, b in enumerate(segs)]
    cut = [e for e in dumped if e[1] == 0 and len(e[3]) >= 3][:24]
    qcaps = [e[3][-1][1] + 1 + s % 9 for s, e in enumerate(cut)]

    def k2(name):
        t = d.k2_targets()[name]
        kind = t["kind"]
        left, _, _ = _run(cuda, t["ins"], d._jc(t["ins"]) if kind == "j" else None, slots=t["slots"], handed=t["handed"], kind=kind,
                          max_len=t.get("max_len"), pad=0, ws_init=sh.t)
        sh.took(left)

    def size(ins, design, **kw):
        keep = []
        z._run_size(cuda, ins, design=design, ws_init=sh.t, keep=keep, **kw)
        sh.took(keep[-1])

    def parts():
        keep = []
        assert p._run_parts(cuda, mixed, design=design, chunks=(256,), ws_init=sh.t, keep=keep)[256][1] > 0
        sh.took(keep[-1])

    def query():
        comp, d_coff, d_ooff, coff, ooff = g._inputs(cuda, [e[2] for e in cut], qcaps)
        idx, sin, sout = g._expected(cut, coff, ooff)
        found, keep = int(idx[-1]), []
        seg_idx, seg_in, seg_out, total = g._query(cuda, comp, d_coff, d_ooff, len(cut), found + 3, ws_init=sh.t, keep=keep)
        assert tuple(total) == (found, found) and np.array_equal(seg_idx, idx)
        assert np.array_equal(seg_in[: found + 1], sin) and np.array_equal(seg_out[: found + 1], sout)
        sh.took(keep[-1])

    def segmented():
        _, st, took = g._decode_both(cuda, segs, caps)
        assert took == "r" and sorted(np.flatnonzero(st != 0)) == [2, 3, 4]

    calls = [lambda: k2("K2r-R6-mixed-wave"), lambda: k2("K2t-T6-deferred"), lambda: k2("K2w-T6-deferred"), lambda: k2("K2j-copies-handed"),
             lambda: size(lane, (1000,), hints=(4096,), route={4096: 1}), lambda: size(wave, (23,), hints=(4097, 1 << 20)), parts, query, segmented,
             lambda: k2("K2t-T7-slots"), lambda: k2("K2r-R4-pairs")]
    for f in calls + calls[::-1]:
        f()


# ------------------------------------------------------------------ three batches whose automatic routes differ


class Batch:
    """A batch of streams on the device with its oracle bytes and the routes it must take."""

    def __init__(self, cuda, name, bufs, max_len, routes):
        self.name, self.max_len, self.routes, self.cuda = name, max_len, routes, cuda
        self.dev = DevBatch(cuda, tuple(bufs))
        self.want = [oracle_bytes(b, MiB, 1024) for b in bufs]
        self.packed_total = sum(len(w) for w in self.want)
        self.longest = int(self.dev.lens.max())

    def run(self, stream):
        return Run(self, stream)


class Run:
    """One K1 -> K3 -> K2 chain of a batch on a stream: every tensor allocated here, up front; the
    three calls only launch."""

    def __init__(self, b, stream):
        import torch

        import eazy_amd as ez

        L, cuda, n = ez._lib(), b.cuda, len(b.want)
        self.b, self.stream = b, stream
        self.cb = b.dev.guarded()
        self.pws_whole, self.pws = dirty.guarded(cuda, L.ez_pack_workspace(n), 0xA5)
        self.packed = torch.full((GUARD + self.cb.slots.numel() + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        self.poff = torch.full((8 + n + 1 + 8,), -7, dtype=torch.int64, device=cuda)
        self.dws_whole, self.dws = dirty.guarded(cuda, L.ez_decompress_workspace(n), 0xA5)
        self.ooff = b.dev.off + GUARD
        self.out = torch.full((GUARD + len(b.dev.host) + GUARD + 16,), FILL, dtype=torch.uint8, device=cuda)
        self.sz = torch.full((n + 2,), -7, dtype=torch.int64, device=cuda)
        self.st = torch.full((n + 2,), -7, dtype=torch.int32, device=cuda)

    def compress(self):
        import eazy_amd as ez

        ez.compress_batch(self.b.dev.data, self.b.dev.off, MiB, 1024, max_len=self.b.max_len, out=self.cb, stream=self.stream)

    def pack(self):
        import eazy_amd as ez

        n = len(self.b.want)
        ez.pack(self.cb, self.packed[GUARD : len(self.packed) - GUARD], self.poff[8 : 8 + n + 1], self.pws, stream=self.stream)

    def decode(self):
        import eazy_amd as ez

        n = len(self.b.want)
        # (the largest slot and both extents given: the decoder is chosen without waiting for the stream)
        ez.decompress_batch(self.packed[GUARD : len(self.packed) - GUARD], self.poff[8 : 8 + n + 1], self.ooff, out=self.out, sizes=self.sz[1 : 1 + n],
                            status=self.st[1 : 1 + n], workspace=self.dws, stream=self.stream, max_len=self.b.longest,
                            in_bytes=self.b.packed_total, out_bytes=len(self.b.dev.host))

    steps = ("compress", "pack", "decode")

    def check(self, what):
        """After the schedule was synchronised."""
        b, n = self.b, len(self.b.want)
        what = f"{what}: batch {b.name}"
        st, sz, off, slots = (t.cpu().numpy() for t in (self.cb.status, self.cb.sizes, self.cb.slot_off, self.cb.slots))
        bad = [s for s, w in enumerate(b.want) if st[s] != 0 or slots[off[s] : off[s] + max(int(sz[s]), 0)].tobytes() != w]
        assert not bad, f"{what}: compressed streams {bad[:8]} differ from the oracle (statuses {st[bad[:8]]})"
        assert (slots[:GUARD] == FILL).all() and (slots[off[-1] :] == FILL).all(), f"{what}: the slots' guards were written"
        poff = self.poff.cpu().numpy()
        assert (poff[:8] == -7).all() and (poff[8 + n + 1 :] == -7).all(), f"{what}: packed_off written outside its entries"
        assert poff[8 : 8 + n + 1].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in b.want])]).tolist(), f"{what}: packed offsets"
        pk = self.packed.cpu().numpy()
        assert pk[GUARD : GUARD + b.packed_total].tobytes() == b"".join(b.want), f"{what}: the packed bytes are not the oracle's"
        assert (pk[:GUARD] == FILL).all() and (pk[GUARD + b.packed_total :] == FILL).all(), f"{what}: bytes outside the packed streams written"
        dirty.guards_intact(self.pws_whole, f"{what}: K3")
        dirty.guards_intact(self.dws_whole, f"{what}: K2")
        dsz, dst = self.sz.cpu().numpy(), self.st.cpu().numpy()
        assert dsz[0] == -7 and dsz[n + 1] == -7 and dst[0] == -7 and dst[n + 1] == -7, f"{what}: results written outside their entries"
        assert not dst[1 : 1 + n].any() and dsz[1 : 1 + n].tolist() == b.dev.lens.tolist(), f"{what}: decode statuses or sizes"
        out = self.out.cpu().numpy()
        assert out[GUARD : GUARD + len(b.dev.host)].tobytes() == b.dev.host.tobytes(), f"{what}: the decoded bytes are not the input"
        assert (out[:GUARD] == FILL).all() and (out[GUARD + len(b.dev.host) :] == FILL).all(), f"{what}: bytes outside the output written"
        assert np.array_equal(b.dev.data.cpu().numpy(), b.dev.host), f"{what}: the input was written"


@pytest.fixture(scope="module")
def batches(cuda):
    """P, Q and R, and the serial pre-run that records and asserts their automatic routes."""
    import torch

    import eazy_amd as ez
    from eazy_amd import synth

    rng = np.random.default_rng(77)
    lens = [0 if s % 37 == 5 else int(rng.integers(1, 4097)) for s in range(300)]
    lens[0], lens[-1] = 4096, 0
    host = synth.logs(31, sum(lens)).tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)])
    p = Batch(cuda, "P", [host[offs[s] : offs[s + 1]] for s in range(300)], 4096, ("s:lean g16 fw40", "r"))
    host = synth.logs(32, 4 << 18).tobytes()
    q = Batch(cuda, "Q", [host[k << 18 : (k + 1) << 18] for k in range(4)], 1 << 18, ("l:k1c", "t"))
    n = MiB + 4099
    host = synth.logs(33, 2 * n).tobytes()
    # (K2j by launch_decompress's automatic rule: at most 256 streams, a slot of 1 MiB or more, at least
    # 64 KiB of input per stream and an output of at least twice the input: the logs compress 2.09 : 1)
    r = Batch(cuda, "R", [host[:n], host[n:]], n, ("x", "j"))
    assert r.max_len > 1 << 19  # (more than half the block: K1s cannot take it, K1x does)
    for b in (p, q, r):
        assert 2 * b.packed_total <= len(b.dev.host) or b.name != "R"
        run = b.run(None)
        torch.cuda.synchronize()
        took = []
        for step in Run.steps:
            getattr(run, step)()
            torch.cuda.synchronize()
            took.append(ez.compress_route_last() if step == "compress" else ez.decompress_kernel_last())
        run.check("serial pre-run")
        assert (took[0], took[2]) == b.routes, (b.name, took)
    return p, q, r


def test_two_streams_one_host_thread(cuda, batches):
    """P on stream A with Q on stream B, call by call (compress P, compress Q, pack P, pack Q, decode
    P, decode Q), then Q on A with R on B, then R on A with P on B: each stream's scratch serves a
    different route from the one that just used it.  Nothing synchronises until the end."""
    import torch

    p, q, r = batches
    a, b = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    pairs = [(x.run(a), y.run(b)) for x, y in ((p, q), (q, r), (r, p))]
    torch.cuda.synchronize()
    for on_a, on_b in pairs:
        for step in Run.steps:
            getattr(on_a, step)()
            getattr(on_b, step)()
    torch.cuda.synchronize()
    for k, (on_a, on_b) in enumerate(pairs):
        on_a.check(f"pair {k}, stream A")
        on_b.check(f"pair {k}, stream B")


def test_two_host_threads(cuda, batches):
    """Two host threads, a stream each, P, Q, R in a different rotation, once: the calls release the
    GIL, so the cache map, the leases and K1c's and K1x's host synchronisations run concurrently."""
    import torch

    p, q, r = batches
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    plans = [[x.run(streams[0]) for x in (p, q, r)], [x.run(streams[1]) for x in (r, p, q)]]
    torch.cuda.synchronize()
    errors = []

    def work(plan):
        try:
            for run in plan:
                for step in Run.steps:
                    getattr(run, step)()
        except BaseException as e:  # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(plan,)) for plan in plans]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k, plan in enumerate(plans):
        for run in plan:
            run.check(f"thread {k}")
