"""K3 (ez_pack.hip: k3_scan1/2/3 and k3_gather) on hand-built slots, K1 not involved.

Every other test hands K3 what K1 just wrote: 16-byte-rounded slots in 256-aligned
allocations, sizes the compressor can produce, at most 65,536 streams.  Here slots, offsets
and sizes are chosen by the test and `ez.pack` is held to plain numpy:

    packed_off = concatenate([0], cumsum(sizes))
    packed     = concatenate(slots[slot_off[s] : slot_off[s] + sizes[s]] for s)

Bar: exact -- offsets equal as int64, bytes as bytes.  Slot bytes are random (not periodic:
a copy shifted by 1-3 bytes cannot pass).  `slots`, `packed`, `packed_off` and the workspace
are views into larger buffers with guards on both sides (the gather reads whole aligned
source dwords, up to 3 bytes either side of a stream; the guards keep those reads inside the
tensor); after every call the guards of `packed`, `packed_off` and the workspace, every byte
of `packed` from packed_off[count] on, and the inputs are checked to be untouched.

P0 (CPU) checks that the case tables cover what they claim; P1 sweeps source residue x
destination residue x size, P2 the split geometry (waves per stream), P3 the scan's tiles and
rounds and the gather's grid-stride loop, P4 packed offsets past 2^32.

The GPU tests are marked one by one (not with a module mark): P0 runs on the CPU."""

import functools

import numpy as np
import pytest

MiB = 1 << 20
GUARD = 64  # bytes either side of every view, inside its buffer
FILL = 0xA5
OFF_FILL = -7  # sentinel of the packed_off buffer
TILE = 1024  # streams per scan tile (ez_pack.hip kTile)
ROUND_TILES = 256  # tiles per k3_scan2 round (kThreads)
MAX_WAVES = 65536 * 4  # k3_gather's grid cap, in waves


def split_of(count):
    """Waves per stream, as launch_pack chooses them."""
    return min(16384 // count, 1024) if count < 16384 else 1


# ------------------------------------------------------------------ batches (host)


class Batch:
    """slots: the bytes of the slots view; stream s = slots[slot_off[s] : slot_off[s] + sizes[s]]."""

    def __init__(self, name, seed, span, slot_off, sizes):
        self.name = name
        self.seed = seed
        self.slot_off = np.asarray(slot_off, np.int64).reshape(-1)
        self.sizes = np.asarray(sizes, np.int64).reshape(-1)
        assert len(self.slot_off) == len(self.sizes)
        self.span = int(span)
        assert self.count == 0 or int((self.slot_off + self.sizes).max()) <= self.span
        self._slots = None
        self._ref = None

    @property
    def count(self):
        return len(self.sizes)

    @property
    def slots(self):
        if self._slots is None:
            self._slots = np.random.default_rng(self.seed).integers(0, 256, self.span, dtype=np.uint8)
        return self._slots

    def reference(self):
        """(packed bytes, packed_off int64[count + 1]); the concatenation of the slices written as
        one fancy index (P0 checks it against the literal concatenation)."""
        if self._ref is None:
            poff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
            idx = np.repeat(self.slot_off - poff[:-1], self.sizes) + np.arange(poff[-1], dtype=np.int64)
            self._ref = (self.slots[idx], poff)
        return self._ref

    def reference_plain(self):
        poff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        parts = [self.slots[o : o + n] for o, n in zip(self.slot_off.tolist(), self.sizes.tolist())]
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), poff

    def geometry(self, src_base, dst_base):
        """Per stream, for views whose addresses are src_base / dst_base mod 4: source residue,
        destination residue, head bytes and body4 (16-byte steps) as k3_gather computes them."""
        _, poff = self.reference()
        sa = (src_base + self.slot_off) & 3
        da = (dst_base + poff[:-1]) & 3
        head = np.minimum((4 - da) & 3, self.sizes)
        body4 = (self.sizes - head) // 16
        return sa, da, head, body4


def cycling_layout(sizes):
    """Slot offsets with source residue s & 3 for stream s and 0-6 unused bytes between slots."""
    sizes = np.asarray(sizes, np.int64)
    blocks = (sizes + 3 + 3) // 4  # dwords that hold residue + size bytes
    start = np.concatenate([[0], np.cumsum(blocks)])
    slot_off = 4 * start[:-1] + (np.arange(len(sizes)) & 3)
    return slot_off, 4 * int(start[-1])


def ragged_gap_layout(sizes, rng):
    """Slot offsets with 0-3 unused bytes before each slot (gap 0 among them)."""
    sizes = np.asarray(sizes, np.int64)
    gaps = rng.integers(0, 4, len(sizes))
    ends = np.cumsum(sizes + gaps)
    return ends - sizes, int(ends[-1]) if len(sizes) else 0


# ---- P1: the alignment x size sweep

SWEEP_SIZES = tuple(range(0, 161)) + (255, 256, 257) + tuple(range(1023, 1041))
SUBSET_SIZES = tuple(range(0, 128))


def steered(name, seed, sizes_wanted, passes):
    """For every pass, every size n of sizes_wanted and every (source residue a, destination
    residue b): a filler stream of 0-3 bytes that brings the packed position to b mod 4, then the
    stream of n bytes at a slot offset of a mod 4.  Slots are laid out in stream order, each at the
    first offset with the wanted residue, so many follow their neighbour with gap 0.  The first
    pass walks the triples in order, later ones in a shuffled order (other neighbours)."""
    rng = np.random.default_rng(seed)
    triples = [(a, b, n) for n in sizes_wanted for a in range(4) for b in range(4)]
    slot_off, sizes = [], []
    c = 0  # end of the last slot
    d = 0  # packed position
    for p in range(passes):
        order = range(len(triples)) if p == 0 else rng.permutation(len(triples)).tolist()
        for t in order:
            a, b, n = triples[t]
            f = (b - d) & 3
            slot_off.append(c)  # the filler: directly after its neighbour
            sizes.append(f)
            c += f
            d += f
            o = c + ((a - c) & 3)
            slot_off.append(o)
            sizes.append(n)
            c = o + n
            d += n
    return Batch(name, seed, c, slot_off, sizes)


@functools.lru_cache(maxsize=None)
def sweep_batch():
    """11,648 streams (split 1): every triple twice."""
    return steered("sweep", 301, SWEEP_SIZES, 2)


@functools.lru_cache(maxsize=None)
def subset_batch():
    """4,096 streams (split 4): sizes 0..127, so parts 1-3 of every stream are idle or nearly."""
    return steered("subset", 302, SUBSET_SIZES, 1)


# ---- P2: split geometry

P2_SPLIT = {1: 1024, 2: 1024, 16: 1024, 17: 963, 100: 163, 5461: 3, 5462: 2, 16383: 1, 16384: 1, 16385: 1}
# count -> per batch of that count, the planted (index, size) pairs; the other streams are ragged
P2_PLANTED = {
    1: ([(0, MiB + 3 * 1024 + 7)], [(0, MiB - 1)], [(0, 45)]),
    2: ([(0, MiB + 5000 + 3), (1, 37)],),
    16: ([(5, MiB + 70001), (11, 9)],),
    17: ([(3, 963 * 64 * 16 + 99), (16, 5)],),
    100: ([(42, 163 * 64 * 16 + 555), (99, 2 * 163 * 64 * 16 + 3)],),
    5461: ([(0, 3 * 1024 + 200), (2730, 3 * 3 * 1024 + 1), (5460, 3 * 1024 + 17)],),
    5462: ([(1, 2 * 1024 + 200), (2731, 3 * 2 * 1024 + 1), (5461, 2 * 1024 + 17)],),
    16383: ([(7, 1024 + 300), (16382, 2 * 1024 + 5)],),
    16384: ([(7, 1024 + 300), (16383, 2 * 1024 + 5)],),
    16385: ([(7, 1024 + 300), (16384, 2 * 1024 + 5)],),
}
P2_CASES = [(count, k) for count in P2_SPLIT for k in range(len(P2_PLANTED[count]))]


@functools.lru_cache(maxsize=None)
def p2_batch(count, k):
    """Ragged sizes (small counts 0..3000 bytes; large counts 0..400 with every 37th 1000..5000),
    the planted streams of P2_PLANTED, source residues cycling."""
    rng = np.random.default_rng(400 + 7 * count + k)
    if count <= 100:
        sizes = rng.integers(0, 3001, count)
    else:
        sizes = rng.integers(0, 401, count)
        sizes[::37] = rng.integers(1000, 5001, len(sizes[::37]))
    for s, n in P2_PLANTED[count][k]:
        sizes[s] = n
    slot_off, span = cycling_layout(sizes)
    assert span < 8 * MiB
    return Batch(f"p2-{count}-{k}", 500 + 7 * count + k, span, slot_off, sizes)


# ---- P3: the scan

P3_COUNTS = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 262143, 262144, 262145, 262144 + 1025, 600001)
BIG = 5000


def p3_planted(count):
    """(zero tile or None, indices that hold BIG): a tile's first index, a tile's last index,
    the very last stream; past one scan2 round also either side of the round's boundary."""
    tiles = -(-count // TILE)
    zero_tile = tiles // 2 if tiles >= 3 else None
    big = set()
    if count:
        big.update((0, count - 1))
    if count >= TILE:
        big.add(TILE - 1)
    if tiles >= 2:
        big.add((tiles - 1) * TILE)  # first index of the last tile
    if tiles >= 4:
        big.add((tiles - 2) * TILE - 1)  # last index of a tile strictly inside
    if count >= ROUND_TILES * TILE:
        big.add(ROUND_TILES * TILE - 1)
    if count > ROUND_TILES * TILE:
        big.add(ROUND_TILES * TILE)
    return zero_tile, sorted(big)


@functools.lru_cache(maxsize=None)
def p3_batch(count):
    rng = np.random.default_rng(600 + count)
    sizes = rng.integers(0, 8, count)
    zero_tile, big = p3_planted(count)
    if zero_tile is not None:
        sizes[zero_tile * TILE : (zero_tile + 1) * TILE] = 0
    for s in big:
        sizes[s] = BIG
    slot_off, span = ragged_gap_layout(sizes, rng)
    return Batch(f"p3-{count}", 700 + count, max(span, 256), slot_off, sizes)


# ------------------------------------------------------------------ P0 (CPU)


def triples_covered(b, src_base, dst_base, sizes_wanted):
    sa, da, _, _ = b.geometry(src_base, dst_base)
    seen = set(zip(sa.tolist(), da.tolist(), b.sizes.tolist()))
    return [(a, d, n) for n in sizes_wanted for a in range(4) for d in range(4) if (a, d, n) not in seen]


def adjacency(b):
    """(slots directly adjacent to the next with gap 0, both non-empty; zero-size streams between
    two non-empty ones)."""
    end = b.slot_off + b.sizes
    gap0 = int(((end[:-1] == b.slot_off[1:]) & (b.sizes[:-1] > 0) & (b.sizes[1:] > 0)).sum())
    z = int(((b.sizes[1:-1] == 0) & (b.sizes[:-2] > 0) & (b.sizes[2:] > 0)).sum())
    return gap0, z


@pytest.mark.parametrize("dst_base", range(4))
@pytest.mark.parametrize("src_base", range(4))
def test_p0_sweep_tables_cover_their_claims(src_base, dst_base):
    """CPU: whatever the views' addresses are mod 4, the P1 batches hold every (source address
    mod 4, destination address mod 4, n) for their sizes, a slot directly adjacent to the next,
    and a zero-size stream between two non-empty ones; the sweep runs with split 1, the subset
    with split 4."""
    for b, wanted, split in ((sweep_batch(), SWEEP_SIZES, 1), (subset_batch(), SUBSET_SIZES, 4)):
        assert split_of(b.count) == split, (b.name, b.count)
        missing = triples_covered(b, src_base, dst_base, wanted)
        assert not missing, f"{b.name}: {len(missing)} triples missing, first {missing[:3]}"
        gap0, z = adjacency(b)
        assert gap0 >= 1 and z >= 1, (b.name, gap0, z)
        # slots do not overlap and lie in stream order
        assert (b.slot_off[1:] >= (b.slot_off + b.sizes)[:-1]).all()
    assert set(SWEEP_SIZES) >= set(range(161)) | {255, 256, 257} | set(range(1023, 1041))
    assert subset_batch().count == 4096 and 8192 < sweep_batch().count < 16384


def test_p0_reference_is_the_plain_concatenation():
    """CPU: the indexed form of the reference equals the literal concatenation of the slices."""
    for b in (sweep_batch(), subset_batch(), p2_batch(100, 0), p3_batch(2049), p3_batch(0)):
        got, poff = b.reference()
        want, poff2 = b.reference_plain()
        assert poff.dtype == np.int64 and np.array_equal(poff, poff2)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), b.name


@pytest.mark.parametrize("dst_base", range(4))
@pytest.mark.parametrize("src_base", range(4))
def test_p0_split_tables_cover_their_claims(src_base, dst_base):
    """CPU: per count of P2, whatever the addresses mod 4: the split has the listed value; some
    stream has body4 > split * 64 (part 0 takes a second round) and ends strictly inside a round;
    some stream has body4 < 64 (parts above 0 idle); every source residue occurs."""
    assert set(P2_SPLIT) == {1, 2, 16, 17, 100, 5461, 5462, 16383, 16384, 16385}
    for count, split in P2_SPLIT.items():
        assert split_of(count) == split, count
        rnd = split * 64
        second = inside = idle = False
        residues = set()
        for k in range(len(P2_PLANTED[count])):
            b = p2_batch(count, k)
            assert b.count == count and b.span < 8 * MiB
            sa, _, _, body4 = b.geometry(src_base, dst_base)
            residues |= set(sa.tolist())
            live = b.sizes > 0
            second |= bool((body4 > rnd).any())
            inside |= bool(((body4 > rnd) & (body4 % rnd != 0)).any())
            idle |= bool((live & (body4 < 64)).any())
        assert second and inside and idle, (count, second, inside, idle)
        assert count < 4 or residues == {0, 1, 2, 3}, (count, residues)
    # count 1: one stream into its second round, one that ends one step short of a full round
    _, _, head, body4 = p2_batch(1, 1).geometry(src_base, dst_base)
    assert body4[0] == 1024 * 64 - 1, body4


def test_p0_scan_tables_hold_their_plants():
    """CPU: the P3 batches hold a tile of zeros, BIG at a tile's first index, at a tile's last
    index and at the very last stream (each where the count has room for it), and the counts
    either side of a tile, of a scan2 round and of the gather's grid."""
    assert set(P3_COUNTS) >= {0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 262143, 262144, 262145, 262144 + 1025, 600001}
    assert ROUND_TILES * TILE == MAX_WAVES == 262144
    for count in P3_COUNTS:
        b = p3_batch(count)
        assert b.count == count
        zero_tile, big = p3_planted(count)
        if count:
            assert b.sizes[count - 1] == BIG and b.sizes[0] == BIG
        if count >= TILE:
            assert any(s % TILE == TILE - 1 for s in big)
        if count > TILE:
            assert any(s % TILE == 0 and s > 0 for s in big)
        if count >= 2049:
            assert zero_tile is not None and 0 < zero_tile < -(-count // TILE) - 1
            assert not b.sizes[zero_tile * TILE : (zero_tile + 1) * TILE].any()
        if count > 262144:
            assert b.sizes[262143] == BIG and b.sizes[262144] == BIG
        small = np.delete(b.sizes, big) if count else b.sizes
        assert small.size == 0 or (small.max() <= 7 and small.min() == 0)
        gap0, _ = adjacency(b)
        assert count < 1023 or gap0 >= 1


# ------------------------------------------------------------------ the device call


def view_start(t, shift):
    """Offset >= GUARD into the uint8 tensor t at which the address is `shift` mod 4."""
    return GUARD + ((shift - (t.data_ptr() + GUARD)) & 3)


def first_bad_stream(b, got, want, poff):
    i = int(np.flatnonzero(got != want)[0])
    s = int(np.searchsorted(poff, i, side="right") - 1)
    return f"first wrong byte at packed[{i}] (got {got[i]:#04x}, expected {want[i]:#04x}), stream {s} of {b.sizes[s]} bytes at +{i - poff[s]}"


def run_pack(cuda, b, src_shift=0, dst_shift=0, covers=None, ws_init=None):
    """ez.pack on the batch with the slots view at src_shift and the packed view at dst_shift
    mod 4 -> asserts the reference's offsets and bytes and that nothing else was written.
    ws_init: a tensor whose first bytes the workspace holds when the call starts (an earlier pack's
    workspace; None: FILL).  Returns the workspace as the call left it."""
    import torch

    import eazy_amd as ez

    want, want_off = b.reference()
    count, total = b.count, len(want)
    what = f"{b.name} (count {count}, split {split_of(count) if count else 0}, slots {src_shift} / packed {dst_shift} mod 4)"

    sbuf = torch.empty(GUARD + 3 + b.span + GUARD, dtype=torch.uint8, device=cuda)
    s0 = view_start(sbuf, src_shift)
    sbuf_h = np.random.default_rng(b.seed + 1).integers(0, 256, sbuf.numel(), dtype=np.uint8)
    sbuf_h[s0 : s0 + b.span] = b.slots
    sbuf.copy_(torch.from_numpy(sbuf_h))
    slots = sbuf[s0 : s0 + b.span]

    cap = total + 64
    pbuf = torch.full((GUARD + 3 + cap + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    p0 = view_start(pbuf, dst_shift)
    packed = pbuf[p0 : p0 + cap]
    assert slots.data_ptr() & 3 == src_shift and packed.data_ptr() & 3 == dst_shift
    if covers is not None:  # the residues of the real addresses, not of the offsets alone
        missing = triples_covered(b, slots.data_ptr() & 3, packed.data_ptr() & 3, covers)
        assert not missing, f"{what}: triples missing {missing[:3]}"

    nws = ez._lib().ez_pack_workspace(count)
    wbuf = torch.full((GUARD + nws + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    if ws_init is not None:
        n = min(nws, ws_init.numel())
        wbuf[GUARD : GUARD + n].copy_(ws_init[:n])
    obuf = torch.full((8 + count + 1 + 8,), OFF_FILL, dtype=torch.int64, device=cuda)
    slot_off = torch.from_numpy(b.slot_off).to(cuda)
    sizes = torch.from_numpy(b.sizes).to(cuda)

    ez.pack(ez.CompressedBatch(slots, slot_off, sizes, None), packed, obuf[8 : 8 + count + 1], wbuf[GUARD : GUARD + nws])
    torch.cuda.synchronize()

    off = obuf.cpu().numpy()
    assert off.dtype == np.int64
    assert (off[:8] == OFF_FILL).all() and (off[-8:] == OFF_FILL).all(), f"{what}: packed_off written outside its count + 1 entries"
    got_off = off[8:-8]
    if not np.array_equal(got_off, want_off):
        i = int(np.flatnonzero(got_off != want_off)[0])
        raise AssertionError(f"{what}: packed_off[{i}] = {got_off[i]}, the cumsum says {want_off[i]}")
    pb = pbuf.cpu().numpy()
    assert (pb[:p0] == FILL).all(), f"{what}: bytes before packed written"
    got = pb[p0 : p0 + total]
    assert got.tobytes() == want.tobytes(), f"{what}: {first_bad_stream(b, got, want, want_off)}"
    assert (pb[p0 + total : p0 + cap] == FILL).all(), f"{what}: bytes from packed_off[count] on written"
    assert (pb[p0 + cap :] == FILL).all(), f"{what}: bytes after packed written"
    wb = wbuf.cpu().numpy()
    assert (wb[:GUARD] == FILL).all() and (wb[GUARD + nws :] == FILL).all(), f"{what}: workspace guards written"
    assert sbuf.cpu().numpy().tobytes() == sbuf_h.tobytes(), f"{what}: slots changed"
    assert np.array_equal(slot_off.cpu().numpy(), b.slot_off), f"{what}: slot_off changed"
    assert np.array_equal(sizes.cpu().numpy(), b.sizes), f"{what}: sizes changed"
    return wbuf[GUARD : GUARD + nws].clone()


# ------------------------------------------------------------------ P1


@pytest.mark.gpu
@pytest.mark.parametrize("dst_shift", range(4))
@pytest.mark.parametrize("src_shift", range(4))
def test_p1_alignment_size_sweep(cuda, src_shift, dst_shift):
    """Split 1: every (source address mod 4, destination address mod 4, n), n in 0..160, 255..257,
    1023..1040 -- n < head, body 0, body4 0, body % 4 != 0 and the wlast clamp one byte at a time
    -- with the slots and the packed view each at every byte alignment."""
    run_pack(cuda, sweep_batch(), src_shift, dst_shift, covers=SWEEP_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("src_shift,dst_shift", [(0, 0), (1, 3), (2, 1), (3, 2)])
def test_p1_small_sizes_with_idle_parts(cuda, src_shift, dst_shift):
    """Split 4 over 4,096 streams of 0..127 bytes: parts 1-3 find nothing or a few steps."""
    run_pack(cuda, subset_batch(), src_shift, dst_shift, covers=SUBSET_SIZES)


@pytest.mark.gpu
def test_p1_slots_in_any_order(cuda):
    """The subset's streams in a shuffled order: the slots no longer lie in stream order."""
    b = subset_batch()
    perm = np.random.default_rng(303).permutation(b.count)
    run_pack(cuda, Batch("shuffled", b.seed, b.span, b.slot_off[perm], b.sizes[perm]), 3, 1)


# ------------------------------------------------------------------ P2


@pytest.mark.gpu
@pytest.mark.parametrize("count,k", P2_CASES, ids=[f"{c}-{k}" for c, k in P2_CASES])
def test_p2_split_geometry(cuda, count, k):
    """Counts either side of every split value launch_pack can choose (1024, 963, 163, 3, 2, 1 and
    the count that leaves the split branch): streams into part 0's second round, ending inside
    a round, and too short for parts above 0; both views off dword alignment."""
    run_pack(cuda, p2_batch(count, k), src_shift=(1 + count + k) & 3, dst_shift=(3 + k) & 3)


# ------------------------------------------------------------------ P3


@pytest.mark.gpu
@pytest.mark.parametrize("count", P3_COUNTS)
def test_p3_scan_and_grid_stride(cuda, count):
    """packed_off over all count + 1 entries and the packed bytes, for counts either side of a
    tile (1,024), of a scan2 round (262,144 streams = 256 tiles) and of the gather's grid
    (262,144 waves); count 0 writes packed_off[0] = 0 and nothing else."""
    run_pack(cuda, p3_batch(count), src_shift=count & 3, dst_shift=(count >> 2) & 3)


# ------------------------------------------------------------------ P4

P4_COUNT = 72
P4_REGION = 64 * MiB


@pytest.mark.gpu
def test_p4_offsets_past_4gib(cuda):
    """72 streams of 64 MiB - s bytes, all read from one 64 MiB region at residues s & 3 (the
    source is const: overlapping slots are legal): about 4.5 GiB packed, so packed_off and the
    gather's destination cross 2^32.  Bytes are compared on the device, stream by stream."""
    import torch

    import eazy_amd as ez

    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free, the test wants 12")
    sizes_h = P4_REGION - np.arange(P4_COUNT, dtype=np.int64)
    slot_off_h = np.arange(P4_COUNT, dtype=np.int64) & 3
    want_off = np.concatenate([[0], np.cumsum(sizes_h)]).astype(np.int64)
    total = int(want_off[-1])
    assert total > 1 << 32 and want_off[P4_COUNT - 9] < 1 << 32  # streams on either side of 4 GiB
    span = P4_REGION + 3

    sbuf_h = np.random.default_rng(801).integers(0, 256, GUARD + 3 + span + GUARD, dtype=np.uint8)
    sbuf = torch.from_numpy(sbuf_h).to(cuda)
    s0 = view_start(sbuf, 2)
    slots = sbuf[s0 : s0 + span]
    keep = sbuf.clone()
    cap = total + 64
    pbuf = torch.full((GUARD + 3 + cap + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    p0 = view_start(pbuf, 1)
    packed = pbuf[p0 : p0 + cap]
    assert slots.data_ptr() & 3 == 2 and packed.data_ptr() & 3 == 1
    nws = ez._lib().ez_pack_workspace(P4_COUNT)
    wbuf = torch.full((GUARD + nws + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    obuf = torch.full((8 + P4_COUNT + 1 + 8,), OFF_FILL, dtype=torch.int64, device=cuda)
    slot_off = torch.from_numpy(slot_off_h).to(cuda)
    sizes = torch.from_numpy(sizes_h).to(cuda)
    try:
        ez.pack(ez.CompressedBatch(slots, slot_off, sizes, None), packed, obuf[8 : 8 + P4_COUNT + 1], wbuf[GUARD : GUARD + nws])
        torch.cuda.synchronize()
        off = obuf.cpu().numpy()
        assert (off[:8] == OFF_FILL).all() and (off[-8:] == OFF_FILL).all()
        assert off.dtype == np.int64 and np.array_equal(off[8:-8], want_off), "packed_off differs from the cumsum"
        for s in range(P4_COUNT):
            o, n, p = int(slot_off_h[s]), int(sizes_h[s]), int(want_off[s])
            assert torch.equal(packed[p : p + n], slots[o : o + n]), f"stream {s} at packed offset {p} differs"
        assert bool((pbuf[:p0] == FILL).all()), "bytes before packed written"
        assert bool((pbuf[p0 + total :] == FILL).all()), "bytes from packed_off[count] on written"
        wb = wbuf.cpu().numpy()
        assert (wb[:GUARD] == FILL).all() and (wb[GUARD + nws :] == FILL).all()
        assert torch.equal(sbuf, keep), "slots changed"
        assert np.array_equal(slot_off.cpu().numpy(), slot_off_h) and np.array_equal(sizes.cpu().numpy(), sizes_h)
    finally:
        del pbuf, packed
        torch.cuda.empty_cache()
