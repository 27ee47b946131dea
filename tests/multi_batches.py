"""Batches for the multi-device host calls (ez_compress_batch_multi, ez_decompressed_size_batch_multi,
ez_decompress_batch_multi) and the checks their tests share.

TEST INFRASTRUCTURE ONLY.  The calls cut a batch into contiguous shards of whole streams by the rule of
eazy_amd/csrc/ez_multi_shards.h: shard k begins with the first stream that starts at or after k / nshard
of the batch's bytes.  ref_bounds states that rule in Python integers; the builders choose stream
lengths that put a stream start on, one byte before and one byte after such a target, empty streams on
it, one stream that outweighs several shards, and streams that do not end cleanly at a shard's first and
last position.  tests/test_gpu_multi_edges.py asserts from the offsets that each batch is what it
claims (no GPU) and then runs the calls.

Nothing expected comes from the library.  Compressed bytes are the C oracle's, stream by stream
(oracle.compress); decoded bytes, sizes and statuses are the oracle Reader's read to EOF
(k2_streams._oracle).  On this host path the bytes of a slot past out_size[s] are unspecified, so only
[0, out_size[s]) of a slot is compared.  Every host array a call writes (packed, packed_off, status,
out, out_size) lies between two 64-byte guards of its fill byte, checked after the call; the calls are
reached through ctypes because the Python wrappers allocate their own outputs."""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import oracle as orc
from k2_streams import HDR, HDR_1K, META_BREAK, META_RESET, _oracle, _slot, cpy, lit, lit_to, meta

MiB = 1 << 20
GUARD = 64
OK, EINVAL, ENOSPC = 0, 12, 14
F_NO_MAGIC = 0x1


# ------------------------------------------------------------------ the rule


def ref_bounds(off, nshard):
    """first[0..nshard]: shard k is streams [first[k], first[k + 1]); first[k] is the first stream with
    (off[s] - off[0]) / total >= k / nshard, in exact integers, or count when there is none."""
    off = [int(x) for x in off]
    count, total = len(off) - 1, off[-1] - off[0]
    first = [0]
    for k in range(1, nshard):
        first.append(next((s for s in range(count) if (off[s] - off[0]) * nshard >= total * k), count))
    return first + [count]


def offsets(streams, lead=0):
    return np.concatenate([[lead], lead + np.cumsum([len(b) for b in streams], dtype=np.int64)]).astype(np.uint64)


def shard_hints(off, nshard):
    """[(longest stream, count)] per shard by the rule."""
    first = ref_bounds(off, nshard)
    n = np.diff(np.asarray(off).astype(np.int64))
    return [(int(n[a:b].max()) if b > a else 0, b - a) for a, b in zip(first, first[1:])]


# ------------------------------------------------------------------ stream lengths


def boundary_lens(nshard, where, empties=0):
    """Lengths of 120 * nshard bytes in pairs of 60 + d and 60 - d, so that the target k / nshard is byte
    120 k.  where = "on": a pair, and so a stream, starts on every target.  "before": a stream starts one
    byte before each target (it belongs to the earlier shard) and none on it; "after": one byte after
    it, and none on it.  empties: that many empty streams start on every target (between a 1-byte
    stream and the pair for "before" and "after", which puts a non-empty start on the target too); they
    belong to the later shard."""
    lens = []
    for k in range(nshard):
        d = 7 + 3 * k
        a, b = 60 + d, 60 - d
        if k:
            if where == "before":
                lens[-1] -= 1
                if empties:
                    lens += [1] + [0] * empties
                else:
                    a += 1
            elif where == "after":
                if empties:
                    lens += [0] * empties + [1]
                else:
                    lens[-1] += 1
                a -= 1
            else:
                lens += [0] * empties
        lens += [a, b]
    assert sum(lens) == 120 * nshard
    return lens


BOUNDARY_NSHARD = (2, 3, 4, 7)
BOUNDARY_WHERE = ("on", "before", "after")
BOUNDARY_EMPTIES = (0, 1, 3)


def boundary_claims(off, nshard, where, empties):
    """Asserts from the offsets alone what boundary_lens says of the batch; returns the bounds."""
    off = [int(x) for x in off]
    first = ref_bounds(off, nshard)
    total = off[-1] - off[0]
    assert total % nshard == 0
    for k in range(1, nshard):
        target = off[0] + total * k // nshard
        f = first[k]
        starts_on = [s for s in range(len(off) - 1) if off[s] == target]
        assert first[k - 1] < f < first[k + 1], (k, first)  # (no shard is empty)
        if where == "on" or empties:
            assert starts_on and f == starts_on[0] and off[f - 1] < target, (k, f)
        else:
            assert not starts_on, k
        if where == "before":
            s = off.index(target - 1)
            assert s < f and off[s + 1] > off[s], (k, s, f)  # a non-empty stream of the earlier shard
        if where == "after":
            s = off.index(target + 1)
            assert f <= s < first[k + 1] and off[s - 1] <= target, (k, s, f)
            if not empties:
                assert s == f
        if empties:
            assert all(off[f + j] == off[f + j + 1] == target for j in range(empties)), k  # empty, on the target,
            assert f + empties <= first[k + 1]  # and of the later shard
            assert off[f + empties + 1] > target
    return first


def heavy_lens(where):
    """One stream of 40,000 bytes among 60 of 100: "front", "middle", "end"."""
    lens = [100] * 60
    lens.insert({"front": 0, "middle": 30, "end": 60}[where], 40000)
    return lens


HEAVY_FIRST = {"front": [0, 1, 1, 1, 61], "middle": [0, 31, 31, 31, 61], "end": [0, 61, 61, 61, 61]}  # on 4 shards


def routes_lens(small=240):
    """Two streams of 70,000 bytes at the ends and `small` of 300 bytes between them.  On 3 shards the
    outer shards hold one long stream each and the middle one the short ones only when the short ones
    together are no fewer bytes than a long one: with 200 of them the last long stream starts before 2/3
    of the bytes, the middle shard takes it and the last shard is empty; with 240 it starts after."""
    return [70000] + [300] * small + [70000]


# ------------------------------------------------------------------ streams


@functools.lru_cache(maxsize=None)
def _logs(seed, n):
    from eazy_amd import synth

    return synth.logs(seed, n).tobytes()


def plain_streams(lens, seed=5):
    """Log text cut into streams of the given lengths."""
    text, out, at = _logs(seed, max(int(sum(lens)), 1)), [], 0
    for n in lens:
        out.append(text[at : at + n])
        at += n
    return out


def exact_streams(lens, seed=9):
    """Compressed streams of exactly the given lengths, for a decode batch with the same offsets as a
    compress batch: the header and literals (k2_streams.lit_to); under 12 bytes, padding bytes only."""
    rng = np.random.default_rng(seed)
    return [lit_to(HDR, n, rng) if n >= 12 else bytes(n) for n in lens]


@functools.lru_cache(maxsize=None)
def want_compressed(block, htable, magic, p):
    return orc.compress(block, htable, [p], append_magic=magic)


def compressed(plains, block=MiB, htable=1024, magic=True):
    return [want_compressed(block, htable, magic, p) for p in plains]


# streams that do not end cleanly (k2_streams' pieces), by name
def odd_streams():
    clean = want_compressed(MiB, 1024, True, _logs(23, 3000))
    return {
        "truncated": clean[: len(clean) - 9],
        "distance-past-window": HDR_1K + lit(bytes(2000)) + cpy(1500, 20) + lit(b"q"),
        "bad-magic": b"\x80\x02eazz" + HDR[6:] + lit(b"abc"),
        "unsupported-meta": HDR + lit(b"abc") + meta(5 << 3, b"x") + lit(b"d"),
        "three-breaks": HDR + lit(b"one") + meta(META_BREAK) + lit(b"two") + meta(META_BREAK) + meta(META_BREAK) + lit(b"three"),
        "reset-after-output": HDR + lit(b"a") + meta(META_RESET, b"\x14") + lit(b"b"),
        "header-only": HDR,
        "empty": b"",
    }


# what the oracle must make of them: (status, decoded bytes)
ODD_WANT = {
    "truncated": (3, None), "distance-past-window": (4, 2000), "bad-magic": (5, 0), "unsupported-meta": (8, 3),
    "three-breaks": (0, 11), "reset-after-output": (0, 2), "header-only": (0, 0), "empty": (0, 0),
}  # fmt: skip


def clean_streams(count=30, seed=31, block=MiB, htable=1024):
    rng = np.random.default_rng(seed)
    return compressed(plain_streams([int(x) for x in rng.integers(200, 600, count)], seed), block, htable)


@functools.lru_cache(maxsize=None)
def place(odd, pos, nshard=3):
    """Clean log streams with `odd` as the first ("first") or last ("last") stream of the middle shard of
    nshard; -> (streams, its index).  An empty stream starts where its successor starts, so it ends no
    shard but the last one: pos = "last" puts an empty stream at the batch's end."""
    k = nshard // 2
    if pos == "last" and not odd:
        return clean_streams() + [odd], len(clean_streams())
    for drop in range(30, -1, -1):  # (all 30 clean streams, or all but one: some choice puts a short stream's few bytes across the target)
        clean = [c for s, c in enumerate(clean_streams()) if s != drop]
        for p in range(1, len(clean)):
            ins = clean[:p] + [odd] + clean[p:]
            first = ref_bounds(offsets(ins), nshard)
            if (pos == "first" and first[k] == p and first[k + 1] > p + 1) or (pos == "last" and first[k + 1] == p + 1 and first[k] < p):
                return ins, p
    raise AssertionError(("no place", len(odd), pos))


LIMIT = 1024  # BlockSizeLimit: the clean streams' block, so none of their tokens is longer; one literal of each stream below is


@functools.lru_cache(maxsize=None)
def limit_batch(nshard=3):
    """Clean log streams with one stream whose second literal is longer than LIMIT as the first stream
    of the middle shard and another as its last; -> (streams, the two indices)."""
    rng = np.random.default_rng(47)
    a = HDR_1K + lit(b"first") + lit(rng.integers(0, 256, LIMIT + 1, dtype=np.uint8).tobytes()) + lit(b"x")
    b = HDR_1K + lit(b"the last") + lit(rng.integers(0, 256, LIMIT + 200, dtype=np.uint8).tobytes())
    clean, k = clean_streams(block=LIMIT, htable=64), nshard // 2
    for p in range(1, len(clean)):
        for q in range(p + 1, len(clean)):
            ins = clean[:p] + [a] + clean[p:q] + [b] + clean[q:]
            first = ref_bounds(offsets(ins), nshard)
            if first[k] == p and first[k + 1] == q + 2:
                return ins, (p, q + 1)
    raise AssertionError("no place")


# ------------------------------------------------------------------ guarded host arrays


class Guarded:
    """n items of dtype, filled with `fill`, between two guards of GUARD bytes of `fill`."""

    def __init__(self, dtype, n, fill):
        size = int(n) * np.dtype(dtype).itemsize
        self.fill = fill
        self.raw = np.full(GUARD + size + GUARD, fill, np.uint8)
        self.a = self.raw[GUARD : GUARD + size].view(dtype)
        self.ptr = self.raw.ctypes.data + GUARD

    def intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[len(self.raw) - GUARD :] == self.fill).all())

    def untouched(self):
        return bool((self.raw == self.fill).all())


def lay(streams, lead=0):
    """The streams back to back after `lead` bytes that must not matter, 16 more after them."""
    rng = np.random.default_rng(len(streams) + lead)
    data = np.concatenate([rng.integers(0, 256, lead, dtype=np.uint8), np.frombuffer(b"".join(streams), np.uint8),
                           rng.integers(0, 256, 16, dtype=np.uint8)])
    return data, offsets(streams, lead)


def _lib():
    import eazy_amd as ez

    L = ez._lib()
    vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
    L.ez_compress_batch_multi.argtypes = [i64, i64, C.c_int, vp, vp, u64, vp, C.c_int, vp, u64, vp, vp]
    L.ez_decompress_batch_multi.argtypes = [i64, vp, vp, u64, vp, C.c_int, vp, vp, vp, vp]
    L.ez_decompressed_size_batch_multi.argtypes = [i64, vp, vp, u64, vp, C.c_int, vp, vp]
    L.ez_multi_last_shards.argtypes = [vp, vp, vp, C.c_int]
    return L


def _devs(devs):
    return (None, 0) if devs is None else ((C.c_int * len(devs))(*devs), len(devs))


# ------------------------------------------------------------------ the three calls, held to the oracle


def _shards_are(off, devs):
    """The shards themselves are invisible in a call's results; their number is not: ez_multi_last_shards
    counts the shards that hold streams, which a start put on the wrong side of a target changes
    wherever a shard holds one stream."""
    if devs is not None:
        want = sum(c > 0 for _, c in shard_hints(off, len(devs)))
        got = _lib().ez_multi_last_shards(None, None, None, 0)
        assert got == want, f"{got} shards held streams, {want} by the rule"


def run_compress(plains, devs, block=MiB, htable=1024, flags=0, lead=0, cap=None, with_status=True, expect=OK):
    """ez_compress_batch_multi on the streams; expect = OK: packed_off, the packed bytes and the statuses
    are the oracle's and nothing else is written; ENOSPC (cap below the oracle's total): packed_off is the
    oracle's and packed untouched; EINVAL: everything untouched.  -> the oracle's streams."""
    want = compressed(plains, block, htable, not (flags & F_NO_MAGIC))
    want_off = offsets(want)
    total, count = int(want_off[-1]), len(plains)
    cap = total + 37 if cap is None else cap
    data, off = lay(plains, lead)
    before = data.copy()
    packed, poff, status = Guarded(np.uint8, cap, 0xC3), Guarded(np.uint64, count + 1, 0x5A), Guarded(np.int32, count, 0x5A)
    d, nd = _devs(devs)
    rc = _lib().ez_compress_batch_multi(block, htable, flags, data.ctypes.data, off.ctypes.data, count, d, nd, packed.ptr, cap, poff.ptr,
                                        status.ptr if with_status else None)
    assert rc == expect, (rc, expect)
    assert packed.intact() and poff.intact() and status.intact(), "a guard was written"
    assert np.array_equal(data, before), "the input was written"
    if not with_status:
        assert status.untouched()
    if expect == EINVAL:
        assert packed.untouched() and poff.untouched() and status.untouched()
        return want
    assert poff.a.tolist() == want_off.tolist(), [(s, int(a), int(b)) for s, (a, b) in enumerate(zip(poff.a, want_off)) if a != b][:4]
    if count:
        _shards_are(off, devs)
    if expect == ENOSPC:
        assert packed.untouched(), "packed was written by a call that returned EZ_ENOSPC"
        return want
    if with_status:
        assert not status.a.any(), status.a.nonzero()[0][:8]
    got = packed.a[:total].tobytes()
    for s in range(count):
        a, b = int(want_off[s]), int(want_off[s + 1])
        assert got[a:b] == want[s], f"stream {s} of {count}: packed bytes differ from the oracle's"
    assert (packed.a[total:] == 0xC3).all(), "bytes past packed_off[count] were written"
    return want


def want_decoded(comps, limit=0, slots=None):
    """[(bytes, status)] of the oracle's Reader read to EOF (slots: each stream's capacity)."""
    return [_oracle(b, slots[s] if slots else max(MiB, 4 * len(b)), limit) for s, b in enumerate(comps)]


def run_sizes(comps, devs, limit=0, lead=0, with_status=True, expect=OK):
    """ez_decompressed_size_batch_multi on the streams: sizes and statuses are the oracle's."""
    count = len(comps)
    data, off = lay(comps, lead)
    before = data.copy()
    size, status = Guarded(np.uint64, count, 0x5A), Guarded(np.int32, count, 0x5A)
    d, nd = _devs(devs)
    rc = _lib().ez_decompressed_size_batch_multi(limit, data.ctypes.data, off.ctypes.data, count, d, nd, size.ptr, status.ptr if with_status else None)
    assert rc == expect, (rc, expect)
    assert size.intact() and status.intact(), "a guard was written"
    assert np.array_equal(data, before), "the input was written"
    if not with_status:
        assert status.untouched()
    if expect != OK:
        assert size.untouched() and status.untouched()
        return None
    if count:
        _shards_are(off, devs)
    want = want_decoded(comps, limit)
    assert size.a.tolist() == [len(w) for w, _ in want], [(s, int(a), len(w)) for s, (a, (w, _)) in enumerate(zip(size.a, want)) if a != len(w)][:4]
    if with_status:
        assert status.a.tolist() == [e for _, e in want], [(s, int(a), e) for s, (a, (_, e)) in enumerate(zip(status.a, want)) if a != e][:4]
    return size.a.copy()


def slot_offsets(comps, limit=0, lead=0):
    """Slots of the oracle's length plus 1..5 bytes, never a multiple of 16 (k2_streams._slot)."""
    cap = [_slot(s, len(w)) for s, (w, _) in enumerate(want_decoded(comps, limit))]
    return cap, np.concatenate([[lead], lead + np.cumsum(cap, dtype=np.int64)]).astype(np.uint64)


def run_decode(comps, devs, limit=0, lead=0, out_lead=0, with_status=True, expect=OK):
    """ez_decompress_batch_multi on the streams: sizes, statuses and the first out_size[s] bytes of every
    slot are the oracle's; no byte before out_off[0] or after out_off[count] is written."""
    count = len(comps)
    data, off = lay(comps, lead)
    before = data.copy()
    cap, ooff = slot_offsets(comps, limit, out_lead)
    out = Guarded(np.uint8, int(ooff[-1]) + 23, 0xC3)
    size, status = Guarded(np.uint64, count, 0x5A), Guarded(np.int32, count, 0x5A)
    d, nd = _devs(devs)
    rc = _lib().ez_decompress_batch_multi(limit, data.ctypes.data, off.ctypes.data, count, d, nd, out.ptr, ooff.ctypes.data, size.ptr,
                                          status.ptr if with_status else None)
    assert rc == expect, (rc, expect)
    assert out.intact() and size.intact() and status.intact(), "a guard was written"
    assert np.array_equal(data, before), "the input was written"
    if not with_status:
        assert status.untouched()
    if expect != OK:
        assert out.untouched() and size.untouched() and status.untouched()
        return
    assert (out.a[:out_lead] == 0xC3).all() and (out.a[int(ooff[-1]) :] == 0xC3).all(), "bytes outside the slots were written"
    if count:
        _shards_are(off, devs)
    want = want_decoded(comps, limit, cap)
    got = out.a.tobytes()
    for s, (w, e) in enumerate(want):
        assert e != 2, s  # (every slot holds the oracle's output)
        assert int(size.a[s]) == len(w), (s, int(size.a[s]), len(w))
        if with_status:
            assert int(status.a[s]) == e, (s, int(status.a[s]), e)
        o = int(ooff[s])
        assert got[o : o + len(w)] == w, f"stream {s} of {count}: decoded bytes differ from the oracle's"


def run_all(plains, devs, block=MiB, htable=1024, flags=0, lead=0, out_lead=0, with_status=True):
    """Compress, size and decode, each held to the oracle."""
    comps = run_compress(plains, devs, block, htable, flags, lead, with_status=with_status)
    run_sizes(comps, devs, 0, lead, with_status)
    run_decode(comps, devs, 0, lead, out_lead, with_status)
    return comps


def run_decodes(comps, devs, limit=0, lead=0, out_lead=0, with_status=True):
    run_sizes(comps, devs, limit, lead, with_status)
    run_decode(comps, devs, limit, lead, out_lead, with_status)


def last_shards(cap=None):
    """ez_multi_last_shards into guarded arrays of `cap` entries (None: as many as it reports) -> (n, devs, t0, t1)."""
    L = _lib()
    n = L.ez_multi_last_shards(None, None, None, 0)
    cap = n if cap is None else cap
    dev, t0, t1 = Guarded(np.int32, cap, 0x5A), Guarded(np.float64, cap, 0x5A), Guarded(np.float64, cap, 0x5A)
    got = L.ez_multi_last_shards(dev.ptr, t0.ptr, t1.ptr, cap)
    assert dev.intact() and t0.intact() and t1.intact(), "a guard was written"
    return n, got, dev.a.tolist(), t0.a.tolist(), t1.a.tolist()
