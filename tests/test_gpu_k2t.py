"""K2t (eazy_amd/csrc/ez_decompress_tok.hip) on hand-built streams, against the oracle.

K2t decodes every batch with a slot of 64 KiB or more, one wave per stream: scan windows of 1,024
input positions, rounds of up to 64 tokens within an output budget, copies in batches, an LDS ring
of 4 or 8 KiB.  The encoder's greedy parse never emits padding, Breaks or short copies, never fills
a round to its budget and never chains 64 dependent copies in one; the groups here
(tests/k2t_streams.py) do, on both sides of each constant: the scan window's end and the lane
segments (T1), the round's 64 tokens (T2), budget = R - 1024 - 64 and kTBig = 512 (T3),
ringlo = pos + total - R + 16 (T4), the batch rule need > oa and the redirect search (T5),
kDeferMin and kDefSlots (T6), the slot's end (T7).

Every group runs at both ring sizes: R = 8192 (a batch of at most 3,072 streams with a slot over
4 KiB), R = 4096 with every slot at most 4 KiB (the streams of the group that fit), and R = 4096
with long outputs (the batch padded to 3,300 streams with 20-byte streams, more than stay resident
with 8 KiB rings).  K2t is forced, and k2_streams._run checks: status, size and bytes equal the
oracle's and the exact decoder's, sentinels round every slot, 0xFF round the input view, and the
streams handed over exactly the ones with an error or a slot too small."""

import numpy as np
import pytest

import k2t_streams as k2t
from k2_streams import HDR, _need, _run, assert_valid, lit, rb

pytestmark = pytest.mark.gpu

_FILL = []


def _fillers(n):
    if not _FILL:
        rng = np.random.default_rng(2100)
        _FILL.extend(k2t.filler20(rng) for _ in range(5))
    return [_FILL[k % 5] for k in range(n)]


def _slots(ins, given):
    """Every stream's slot: the given one, else the oracle's length plus 1..5 bytes (an output of
    under 15 bytes gets 17..21: K2t does not take a slot under 16 bytes)."""
    out = {}
    for s, b in enumerate(ins):
        need = _need(b)
        n = need + 1 + s % 5
        out[s] = given[s] if given.get(s) is not None else (17 + s % 5 if need < 15 else (n + 1 if n % 16 == 0 else n))
    return out


def _rings(cuda, named, slots=None, handed="auto", which="ABC"):
    """named: [(name, stream)]; slots: {index: slot}.  The batch at R = 8192 (A), its streams with
    slots of at most 4 KiB at R = 4096 (B), and the batch padded to 3,300 streams at R = 4096 (C)."""
    slots = slots or {}
    ins = [b for _, b in named]
    if "A" in which:
        a = ins + [HDR + lit(rb(np.random.default_rng(2199), 5000))]  # (a slot over 4 KiB)
        assert len(a) <= 3072
        sl = _slots(a, slots)
        assert max(sl.values()) > 4096
        _run(cuda, a, slots=sl, handed=handed, kind="t", max_len=True, pad=0)
    if "B" in which:
        keep = [s for s, b in enumerate(ins) if max(_need(b), slots.get(s) or 0) <= 4080]
        if keep:
            sub = [ins[s] for s in keep]
            sl = _slots(sub, {k: slots.get(s) for k, s in enumerate(keep)})
            assert max(sl.values()) <= 4096
            _run(cuda, sub, slots=sl, handed=handed, kind="t", max_len=True, pad=29)
    if "C" in which:
        c = ins + _fillers(3300 - len(ins))
        assert len(c) == 3300
        _run(cuda, c, slots=_slots(c, slots), handed=handed, kind="t", max_len=True, pad=0)


def test_k2t_scan_seams(cuda):
    """T1: every token form with its header 0 .. header-length bytes before the end of the first scan
    window and of a drifted later one, at every offset mod 16, rare forms back to back, and the
    70,000-byte literal as a window's last token.  No stream is handed over."""
    named = k2t.t1_streams()
    assert_valid(named)
    _rings(cuda, named)


def test_k2t_rounds(cuda):
    """T2: windows of exactly 63, 64, 65, 128 and 512 tokens, a window of 1,024 padding zeros, Breaks
    inside a round, 100 zeros before the header, a reset on another lane than 0; two MetaResets
    before any output (the oracle's result, whoever decodes it)."""
    named = k2t.t2_streams()
    assert_valid(named)
    _rings(cuda, named)
    _rings(cuda, k2t.t2_two_resets(), handed=None)


def test_k2t_budget_and_big_tokens(cuda):
    """T3: tokens of 511, 512 and 513 bytes; rounds reaching budget - 1, budget, budget + 1 (3,008 and
    7,104); a 512-byte token ending exactly on the budget."""
    named = k2t.t3_streams()
    assert_valid(named)
    _rings(cuda, named)


@pytest.mark.parametrize("R", [4096, 8192])
def test_k2t_ring_reach(cuda, R):
    """T4: 200-byte copies with every D in [R - 1104, R + 48], first, in the middle and last in a
    round that fills its budget, over output stamped every 40 bytes: sources on both sides of
    ringlo and straddling it, at the ring size they are built for."""
    named = k2t.t4_streams(R)
    assert len(named) == -(-1153 * 3 // 12)
    assert_valid(named)
    _rings(cuda, named, which="A" if R == 8192 else "C")


def test_k2t_copy_batches(cuda):
    """T5: sources ending at and just past an earlier copy's first byte, D in 15..17 with L > D, 64
    chained copies in a round, and rounds of copies reading the round's own output (redirects once
    and twice deep, sources in a literal, straddling tokens, zero-length tokens between)."""
    named = k2t.t5_streams()
    assert_valid(named)
    _rings(cuda, named)


def test_k2t_alone_and_deferred(cuda):
    """T6: literals of 16,383 / 16,384 / 16,385 bytes, nine deferred-size literals in a stream,
    copies and runs across a deferred literal's first and last byte, 600-byte copies and runs after
    it, and D > pos on the round and the alone path."""
    named = k2t.t6_streams()
    assert_valid(named)
    _rings(cuda, named)


def test_k2t_slots(cuda):
    """T7: the slot exactly enough and one byte short at a token of a round and at a token moved
    alone: ENOSPC with the exact decoder's size, and only those streams handed over."""
    from k2_streams import _oracle

    t7 = k2t.t7_streams()
    named, slots = [], {}
    for name, b, need in t7:
        assert _need(b) == need and _oracle(b, need)[1] == 0 and _oracle(b, need - 1)[1] == 2
        for d in (0, 1):
            slots[len(named)] = need - d
            named.append((f"{name}-{d}", b))
    _rings(cuda, named, slots=slots)
