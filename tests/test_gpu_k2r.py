"""K2r (eazy_amd/csrc/ez_decompress_ring.hip) on hand-built streams, against the oracle.

K2r decodes every batch whose largest slot is under 64 KiB, one lane per stream, with the stream's
last 512 output bytes in an LDS ring.  The streams of the other tests come from the encoder's greedy
parse, which never emits a copy shorter than 6 bytes and never places one at the distance where K2r
switches from the ring to HBM.  The groups here (tests/k2r_streams.py; tests/test_ring_emu.py runs
the same streams through the lane code on the CPU) sit on both sides of every constant the kernel
rests on: kNear = kRing - 16 (R1), ring_st's mirror and guard writes at every ring residue (R2),
runs and zero regions of every period and length (R3), the literal + copy pair rule o2 <= 11 and
16 - o2 - adv2 >= 0 (R4), the clamped loads at the batch's end and the slot's edges (R5), and a
block's worth of lanes holding unlike streams (R6).

Every batch is decoded with K2r forced and once more with the library's own choice (which must be
K2r), and checked by k2_streams._run: status, size and bytes equal the oracle's and the exact
decoder's, the 0xA5 sentinels round every slot intact, 0xFF round the input view, and the streams
handed to the exact decoder exactly the ones with an error or a slot too small."""

import pytest

import k2r_streams as k2r
from k2_streams import _need, _oracle, _run

pytestmark = pytest.mark.gpu


def _go(cuda, cases, limit=0, pads=(0, 37)):
    ins = [c.stream for c in cases]
    # (a default slot under 16 bytes, which K2r does not take, becomes one of 17..21 bytes)
    slots = {s: c.slot if c.slot is not None else 17 + s % 5 for s, c in enumerate(cases) if c.slot is not None or _need(c.stream, limit) < 15}
    handed = k2r.expected_handed([c._replace(slot=slots.get(s)) for s, c in enumerate(cases)], limit)
    for kind, pad in zip(("r", ""), pads):
        _run(cuda, ins, slots=slots, handed=handed, kind=kind, last="r", max_len=True, block_size_limit=limit, pad=pad)
    return handed


def _all_valid(cases):
    for c in cases:
        assert _oracle(c.stream, 1 << 20)[1] == 0, c.name


def test_k2r_ring_hbm_threshold(cuda):
    """R1: copies with D in 481..528 and L in 1..300 after 9..16 pair steps, after a run and after a
    100-byte literal.  D <= 496 reads the ring, D >= 497 the output in HBM while up to kChunk + 31 * 9
    bytes wait in the ring.  No stream is handed over."""
    cases = k2r.r1_streams()
    assert len(cases) == 48 * 8 * 3
    _all_valid(cases)
    assert _go(cuda, cases) == set()


def test_k2r_ring_residues(cuda):
    """R2: a near copy, a far copy, a run and a 15-byte literal stored at every ring residue 0..527."""
    cases = k2r.r2_streams()
    _all_valid(cases)
    assert _go(cuda, cases) == set()


def test_k2r_runs_and_zero_regions(cuda):
    """R3: D in 0..15 and L in 1..48, 123, 124, 379, 380, 1000 at output phases 5, 500 and 509; runs
    reaching before the stream start, first in the stream, after a pair and after a 1-byte literal."""
    cases = k2r.r3_streams()
    _all_valid(cases)
    assert _go(cuda, cases) == set()


def test_k2r_pairs(cuda):
    """R4: L1 in 1..15 before every copy header form and kind; pairs last in the stream; slots exact
    and one byte short (ENOSPC, handed over); D = window + 1 (EOVERFLOW, handed over)."""
    import eazy_amd as ez

    cases = k2r.r4_streams()
    for c in cases:
        if c.slot is None:
            assert _oracle(c.stream, 1 << 20)[1] == (ez.EOVERFLOW if "window-D1025" in c.name else 0), c.name
    handed = _go(cuda, cases)
    assert {cases[s].name.split("-", 2)[2] for s in handed} >= {"window-D1025-off2", "near-plain-slot-1", "zero-slot-1"}
    assert all("window-D1025" in cases[s].name or cases[s].name.endswith("slot-1") for s in handed)


def test_k2r_pairs_block_size_limit(cuda):
    """R4 with BlockSizeLimit = 8: L1 and L2 equal to the limit decode on K2r, one more is
    EBLOCKLIMIT from the exact decoder; D = window + 1 under the 8-byte window is EOVERFLOW."""
    cases = k2r.r4_limit_streams()
    bad = k2r.expected_handed(cases, k2r.R4_LIMIT)
    for s, c in enumerate(cases):
        assert (s in bad) == ("L1_9" in c.name or "L1_10" in c.name or "L2_9" in c.name or "D9" in c.name), c.name
    assert _go(cuda, cases, limit=k2r.R4_LIMIT) == bad


def test_k2r_last_stream_tails(cuda):
    """R5: the batch's last stream ends in a literal of 1..20, 31, 32 or 33 bytes or in a copy header,
    or is shorter than 16 bytes in all; the input view ends right there (0xFF follows)."""
    for name, cases in k2r.r5_last_stream_batches():
        _go(cuda, cases, pads=(0, 0))


def test_k2r_batch_under_16_bytes(cuda):
    """R5: a batch of less than 16 input bytes: every stream is handed over, results the oracle's."""
    for name, cases in k2r.r5_tiny_batches():
        ins = [c.stream for c in cases]
        assert sum(len(b) for b in ins) < 16
        for kind in ("r", ""):
            _run(cuda, ins, handed="all", kind=kind, last="r", max_len=True, pad=0)


def test_k2r_slot_edges(cuda):
    """R5: a first stream whose first token copies from 600 bytes before its start (zeros, not the
    sentinel before out_off[0]); empty and header-only streams; slots of exactly the needed size;
    slots of 15 (handed over), 16 and 17 bytes."""
    cases = k2r.r5_streams()
    assert cases[0].name == "r5-first-far-copy" and _oracle(cases[0].stream, 1 << 20)[0][:50] == bytes(50)
    handed = _go(cuda, cases)
    assert all("slot15" in cases[s].name or "need17-slot16" in cases[s].name or "need18-slot1" in cases[s].name for s in handed)
    assert sum("slot15" in cases[s].name for s in handed) == 6


def test_k2r_mixed_wave(cuda):
    """R6: 327 streams, neighbouring lanes holding an empty stream, a 1-byte output, a 40 KiB
    output, truncated and bit-flipped streams and slots too small: only the invalid and the too-small
    ones are handed over, every other stream is exact."""
    cases = k2r.r6_streams()
    assert len(cases) == 327
    handed = _go(cuda, cases)
    assert all(cases[s].name.split("-")[2] in ("truncated", "bit", "small") for s in handed)
    assert sum(cases[s].name.endswith("small-slot") for s in handed) == sum(c.name.endswith("small-slot") for c in cases)
