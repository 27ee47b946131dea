"""ez_compress_batch_multi, ez_decompressed_size_batch_multi and ez_decompress_batch_multi held to the C
oracle at every shard edge (tests/multi_batches.py builds the batches and holds the calls' outputs,
between guards, to the oracle; eazy_amd/csrc/ez_multi_shards.h is the rule that cuts the shards,
checked on the host by tests/test_multi_shards.py).  Every device list is entries of device 0.

Without a device: the batches are what they claim, read back from their offsets; decreasing offsets
are refused with EZ_EINVAL before any device use and nothing is written.
S1 stream starts on, before and after a shard's target, empty streams on it, one stream that outweighs
   several shards (empty shards in the middle), only empty streams, fewer streams than shards
S2 shards of one call on different K1 routes and different decoders
S3 (block, htable), EZ_F_NO_MAGIC and block_size_limit passed through
S4 in_off[0] and out_off[0] not 0, status == NULL, devices == NULL, device entries that do not exist
S5 EZ_ENOSPC: packed_off filled, packed untouched
S6 streams that do not end cleanly as the first and the last stream of the middle shard
S7 the pooled shard buffers across calls of changing size and shard count, nine shards on one device
S8 two host threads at once
S9 ez_multi_last_shards"""

import ctypes as C
import threading

import numpy as np
import pytest

import multi_batches as mb
from multi_batches import EINVAL, ENOSPC, MiB

BOUNDARY = [(n, w, e) for n in mb.BOUNDARY_NSHARD for w in mb.BOUNDARY_WHERE for e in mb.BOUNDARY_EMPTIES]
ODD = [(name, pos) for name in mb.ODD_WANT for pos in ("first", "last")]


# ------------------------------------------------------------------ without a device


def test_batches_are_what_they_claim():
    for n, where, empties in BOUNDARY:
        lens = mb.boundary_lens(n, where, empties)
        for streams in (mb.plain_streams(lens), mb.exact_streams(lens)):
            assert [len(b) for b in streams] == lens
            for lead in (0, 13):
                mb.boundary_claims(mb.offsets(streams, lead), n, where, empties)
        assert all(e == 0 for _, e in mb.want_decoded(mb.exact_streams(lens))), (n, where, empties)  # (clean streams)
    for n in mb.BOUNDARY_NSHARD:  # one stream per shard, each on its target
        off = mb.offsets(mb.plain_streams([120] * n), 13)
        assert mb.ref_bounds(off, n) == list(range(n + 1)) and all((int(off[k]) - 13) * n == 120 * n * k for k in range(n))
    for where, first in mb.HEAVY_FIRST.items():
        off = mb.offsets(mb.plain_streams(mb.heavy_lens(where)))
        assert mb.ref_bounds(off, 4) == first, where
        assert np.diff(off.astype(np.int64)).tolist().count(40000) == 1
    assert sum(a == b for a, b in zip(mb.HEAVY_FIRST["front"], mb.HEAVY_FIRST["front"][1:])) == 2  # empty shards in the middle
    assert mb.ref_bounds(mb.offsets([b""] * 20, 7), 4) == [0, 0, 0, 0, 20]  # (every stream starts on every target of 0 bytes: the last shard's)
    assert mb.ref_bounds(mb.offsets([b"abc"]), 8) == [0] + [1] * 8
    assert mb.ref_bounds(mb.offsets([b"abc", b"defg"]), 4) == [0, 1, 2, 2, 2]
    # S2: 200 short streams leave the last shard of 3 empty, 240 give the outer shards one long stream each
    assert mb.shard_hints(mb.offsets(mb.plain_streams(mb.routes_lens(200))), 3) == [(70000, 1), (70000, 201), (0, 0)]
    h = mb.shard_hints(mb.offsets(mb.plain_streams(mb.routes_lens(240))), 3)
    assert [mx for mx, _ in h] == [70000, 300, 70000] and h[0][1] < 8 and h[2][1] < 8 and h[1][1] > 200, h
    # S3: two streams over the limit, the middle shard's first and last
    import eazy_amd as ez

    ins, over = mb.limit_batch()
    first = mb.ref_bounds(mb.offsets(ins), 3)
    assert over == (first[1], first[2] - 1) and over[0] < over[1]
    want = mb.want_decoded(ins, mb.LIMIT)
    assert [s for s, (_, e) in enumerate(want) if e != 0] == list(over) and all(want[s][1] == ez.EBLOCKLIMIT for s in over)
    assert [len(want[s][0]) for s in over] == [5, 8] and all(e == 0 for _, e in mb.want_decoded(ins))
    # S6: the odd streams are what their names say, and stand where place() says
    odd = mb.odd_streams()
    assert set(odd) == set(mb.ODD_WANT)
    for name, (status, size) in mb.ODD_WANT.items():
        w, e = mb.want_decoded([odd[name]])[0]
        assert e == status and (size is None or len(w) == size), (name, e, len(w))
    assert 0 < len(mb.want_decoded([odd["truncated"]])[0][0]) < 3000
    for name, pos in ODD:
        ins, p = mb.place(odd[name], pos)
        first = mb.ref_bounds(mb.offsets(ins), 3)
        assert ins[p] == odd[name] and all(e == 0 for s, (_, e) in enumerate(mb.want_decoded(ins)) if s != p)
        if pos == "first":
            assert first[1] == p < first[2] - 1, (name, first, p)
        elif name == "empty":
            assert p == len(ins) - 1 == first[3] - 1 and first[2] < p, (name, first, p)
        else:
            assert first[1] < p == first[2] - 1 < first[3] - 1, (name, first, p)


def test_decreasing_offsets_are_refused_before_any_device_use():
    """A three-stream offset array that decreases once: EZ_EINVAL from each of the three calls, with or
    without a device, and no array written (packed_off[0] neither)."""
    import eazy_amd as ez

    L = mb._lib()
    data = np.zeros(64, np.uint8)
    up = np.array([0, 10, 20, 30], np.uint64)
    for down in (np.array([0, 10, 9, 30], np.uint64), np.array([5, 4, 20, 30], np.uint64), np.array([0, 10, 20, 19], np.uint64)):
        g = {k: mb.Guarded(dt, n, 0x5A) for k, (dt, n) in {"packed": (np.uint8, 256), "poff": (np.uint64, 4), "status": (np.int32, 3),
                                                            "out": (np.uint8, 256), "size": (np.uint64, 3)}.items()}
        devs = (C.c_int * 2)(0, 0)
        assert L.ez_compress_batch_multi(MiB, 1024, 0, data.ctypes.data, down.ctypes.data, 3, devs, 2, g["packed"].ptr, 256, g["poff"].ptr,
                                         g["status"].ptr) == ez.EINVAL
        assert L.ez_decompressed_size_batch_multi(0, data.ctypes.data, down.ctypes.data, 3, devs, 2, g["size"].ptr, g["status"].ptr) == ez.EINVAL
        assert L.ez_decompress_batch_multi(0, data.ctypes.data, down.ctypes.data, 3, devs, 2, g["out"].ptr, up.ctypes.data, g["size"].ptr,
                                           g["status"].ptr) == ez.EINVAL
        assert L.ez_decompress_batch_multi(0, data.ctypes.data, up.ctypes.data, 3, devs, 2, g["out"].ptr, down.ctypes.data, g["size"].ptr,
                                           g["status"].ptr) == ez.EINVAL
        assert L.ez_decompress_batch_multi(0, data.ctypes.data, up.ctypes.data, 3, None, 0, g["out"].ptr, down.ctypes.data, g["size"].ptr,
                                           None) == ez.EINVAL
        assert all(a.untouched() for a in g.values()), [k for k, a in g.items() if not a.untouched()]


# ------------------------------------------------------------------ S1: boundaries


@pytest.mark.gpu
@pytest.mark.parametrize("nshard", mb.BOUNDARY_NSHARD)
def test_s1_stream_starts_at_the_targets(cuda, nshard):
    """A stream start on, one byte before and one byte after every target of nshard shards, without and
    with one and three empty streams on the target: compressed, sized and decoded; and the same offsets as
    compressed streams, sized and decoded.  And one stream per shard, each on its target: a start taken
    for the earlier shard's would leave the last shard without a stream, and every call is held to the
    number of shards that hold streams (ez_multi_last_shards)."""
    mb.run_all(mb.plain_streams([120] * nshard), [0] * nshard, lead=13)
    mb.run_decodes(mb.exact_streams([120] * nshard), [0] * nshard)
    for where in mb.BOUNDARY_WHERE:
        for empties in mb.BOUNDARY_EMPTIES:
            lens = mb.boundary_lens(nshard, where, empties)
            mb.run_all(mb.plain_streams(lens), [0] * nshard)
            mb.run_decodes(mb.exact_streams(lens), [0] * nshard)


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(mb.HEAVY_FIRST))
def test_s1_one_stream_outweighs_several_shards(cuda, where):
    mb.run_all(mb.plain_streams(mb.heavy_lens(where)), [0] * 4)


@pytest.mark.gpu
def test_s1_empty_streams_and_fewer_streams_than_shards(cuda):
    mb.run_all([b""] * 20, [0] * 4)
    mb.run_all([b""] * 20, [0])
    mb.run_all(mb.plain_streams([5000]), [0] * 8)
    mb.run_all(mb.plain_streams([3000, 4000]), [0] * 4)


# ------------------------------------------------------------------ S2: shards on different routes


S2_BLOCK = 65536  # a stream of 70,000 bytes does not fit twice into it (K1x), one of 300 does (K1s)


@pytest.mark.gpu
def test_s2_shards_on_different_routes(cuda):
    """Two streams of 70,000 bytes round 240 of 300 on 3 shards, block 65,536: the outer shards' K1 kernel
    (ez_compress_kernel of each shard's longest stream and count) is not the middle one's, and on the way
    back the outer shards' largest slot is over 64 KiB (a wave per stream) and the middle one's under it
    (a lane per stream).  The same bytes on 2 shards and on 1, and at a block of 1 MiB; and with 200 short
    streams, where the rule leaves the last shard empty."""
    import eazy_amd as ez

    plains = mb.plain_streams(mb.routes_lens(240))
    hints = mb.shard_hints(mb.offsets(plains), 3)
    kernels = [ez.compress_kernel(S2_BLOCK, 1024, mx, c) for mx, c in hints]
    assert kernels[0] == kernels[2] != kernels[1], (hints, kernels)
    comps = mb.compressed(plains, S2_BLOCK, 1024)
    cap, ooff = mb.slot_offsets(comps)
    first = mb.ref_bounds(mb.offsets(comps), 3)
    largest = [max(cap[a:b]) for a, b in zip(first, first[1:])]
    assert largest[1] < 65536 < min(largest[0], largest[2]), largest
    for devs in ([0] * 3, [0] * 2, [0]):
        assert mb.run_all(plains, devs, S2_BLOCK, 1024) == comps
    mb.run_all(plains, [0] * 3)
    mb.run_all(mb.plain_streams(mb.routes_lens(200)), [0] * 3, S2_BLOCK, 1024)
    mb.run_all(mb.plain_streams(mb.routes_lens(200)), [0] * 3)


# ------------------------------------------------------------------ S3: arguments passed through


@pytest.mark.gpu
@pytest.mark.parametrize("block,htable", [(4096, 64), (1024, 16), (65536, 256)])
def test_s3_block_and_table(cuda, block, htable):
    plains = mb.plain_streams(mb.heavy_lens("front"))
    mb.run_all(plains, [0] * 4, block, htable)
    mb.run_all(plains, [0] * 4, block, htable, flags=mb.F_NO_MAGIC)


@pytest.mark.gpu
def test_s3_no_magic_at_the_default_sizes(cuda):
    plains = mb.plain_streams(mb.heavy_lens("front"))
    comps = mb.run_all(plains, [0] * 4, flags=mb.F_NO_MAGIC)
    assert all(not c.startswith(b"\x80\x02eazy") for c in comps) and all(c.startswith(b"\x80\x02eazy") for c in mb.compressed(plains))


@pytest.mark.gpu
def test_s3_block_size_limit(cuda):
    """Clean streams round two with a literal longer than block_size_limit, the middle shard's first and
    last stream: those two are EZ_EBLOCKLIMIT with the oracle's size from the size call and the decode,
    the others exact; without a limit all are clean."""
    ins, _ = mb.limit_batch()
    mb.run_decodes(ins, [0] * 3, limit=mb.LIMIT)
    mb.run_decodes(ins, [0] * 3, limit=0)


# ------------------------------------------------------------------ S4: placement


@pytest.mark.gpu
def test_s4_offsets_that_do_not_start_at_zero(cuda):
    for lens in (mb.boundary_lens(3, "on", 1), mb.heavy_lens("middle")):
        mb.run_all(mb.plain_streams(lens), [0] * 3, lead=13, out_lead=29)
    mb.run_decodes(mb.exact_streams(mb.boundary_lens(4, "before", 0)), [0] * 4, lead=13, out_lead=29)


@pytest.mark.gpu
def test_s4_status_null(cuda):
    mb.run_all(mb.plain_streams(mb.boundary_lens(3, "on", 1)), [0] * 3, with_status=False)
    ins, _ = mb.place(mb.odd_streams()["truncated"], "first")
    mb.run_decodes(ins, [0] * 3, with_status=False)


@pytest.mark.gpu
def test_s4_every_device_of_the_machine(cuda):
    mb.run_all(mb.plain_streams(mb.heavy_lens("middle")), None)
    mb.run_all(mb.plain_streams(mb.boundary_lens(7, "after", 3)), None)


@pytest.mark.gpu
def test_s4_devices_that_do_not_exist(cuda):
    import eazy_amd as ez

    plains = mb.plain_streams(mb.boundary_lens(2, "on", 0))
    for devs in ([-1], [0, -1], [ez.device_count()], [0, ez.device_count()]):
        comps = mb.run_compress(plains, devs, expect=EINVAL)
        mb.run_sizes(comps, devs, expect=EINVAL)
        mb.run_decode(comps, devs, expect=EINVAL)


# ------------------------------------------------------------------ S5: EZ_ENOSPC


@pytest.mark.gpu
def test_s5_enospc(cuda):
    for lens in (mb.heavy_lens("middle"), mb.boundary_lens(4, "on", 1)):
        plains = mb.plain_streams(lens)
        total = sum(len(c) for c in mb.compressed(plains))
        mb.run_compress(plains, [0] * 4, cap=total - 1, expect=ENOSPC)
        mb.run_compress(plains, [0] * 4, cap=total)
    mb.run_compress(mb.plain_streams(mb.heavy_lens("front")), [0] * 4, cap=0, expect=ENOSPC)


# ------------------------------------------------------------------ S6: streams that do not end cleanly


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mb.ODD_WANT))
def test_s6_odd_streams_at_shard_edges(cuda, name):
    for pos in ("first", "last"):
        ins, _ = mb.place(mb.odd_streams()[name], pos)
        mb.run_decodes(ins, [0] * 3)


# ------------------------------------------------------------------ S7: the pool


@pytest.mark.gpu
def test_s7_pool_across_calls_of_changing_size_and_shard_count(cuda):
    """1 MiB on 3 shards, 2 KiB on 1, 300 KiB on 2, then 9 shards on the one device (one more than the
    scratch cache keeps per device, so it frees its least recently used entry while shards run), then
    every idle buffer set to 0xA5 and the first batch again on 2 shards."""
    import eazy_amd as ez

    rng = np.random.default_rng(3)
    big = mb.plain_streams([4096] * 256, 11)
    mb.run_all(big, [0] * 3)
    mb.run_all(mb.plain_streams([256] * 8, 12), [0])
    mb.run_all(mb.plain_streams([int(x) for x in rng.integers(0, 6000, 100)], 13), [0] * 2)
    mb.run_all(mb.plain_streams(mb.boundary_lens(7, "on", 1)), [0] * 9)
    assert ez.fill_cached(0xA5) > 0
    mb.run_all(big, [0] * 2)


# ------------------------------------------------------------------ S8: two host threads


@pytest.mark.gpu
def test_s8_two_host_threads(cuda):
    batches = [mb.plain_streams([1000] * 64, 21), mb.plain_streams([3000] * 40, 22)]
    for plains in batches:  # (both shards of every call hold streams: 2 shards are reported whichever call was last)
        assert all(c for _, c in mb.shard_hints(mb.offsets(plains), 2)) and all(c for _, c in mb.shard_hints(mb.offsets(mb.compressed(plains)), 2))
    start, errors = threading.Barrier(2), []

    def work(plains):
        try:
            start.wait()
            mb.run_all(plains, [0] * 2)
        except BaseException as e:  # noqa: BLE001 (reported by the test's thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(p,)) for p in batches]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    assert mb.last_shards()[0] == 2


# ------------------------------------------------------------------ S9: ez_multi_last_shards


@pytest.mark.gpu
def test_s9_last_shards(cuda):
    plains = mb.plain_streams(mb.heavy_lens("front"))
    mb.run_compress(plains, [0] * 4)
    want = sum(c > 0 for _, c in mb.shard_hints(mb.offsets(plains), 4))
    assert want == 2
    n, got, dev, t0, t1 = mb.last_shards()
    assert n == got == want and dev == [0] * want
    assert all(0 <= a <= b for a, b in zip(t0, t1)), (t0, t1)
    n, got, dev, t0, t1 = mb.last_shards(cap=1)
    assert n == got == want and dev == [0] and 0 <= t0[0] <= t1[0]
    assert mb._lib().ez_multi_last_shards(None, None, None, 4) == want
    mb.run_compress(plains, [0] * 3)  # 3 shards by the rule: the long stream, none, the short ones
    assert mb.last_shards()[0] == sum(c > 0 for _, c in mb.shard_hints(mb.offsets(plains), 3))
