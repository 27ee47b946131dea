"""The steps of K2g's parts route (eazy_amd/csrc/ez_k2_segs_parts.h: a lane's sum of its chunk of the
chain, the join of two sums in chain order, a part's record, the in-order pass that follows the true
chain through the records and leaves every part's entry state, the fill from an entry state),
compiled for the host by tools/k2_segs_parts_check.hip and run over emulated lanes, parts and streams
exactly as the kernels order them, for chunk 256 and chunk 1,024, on hand-built streams of 2 to 6
parts: a Reset at each of the last 8 positions before a part seam and at the first after it; 40 Resets
in one part; 2 and 3 Resets with nothing between them straddling a seam at every offset; leading Resets
before the stream's first output byte across a seam (no cuts), and the same after one output byte (all
cuts); more than 15 cuts in one stream; a literal over exactly one whole part and then a Reset (a part
passed through); literal bodies of 80 10 14, of whole headers and of copy headers across seams (parts
walked again: counted); a segment over three parts with a distance past its window (the stop lands in a
later part, later Resets are no cuts) and with its longest distance exactly its window; a hand-over
form in one part with Resets in the next; an error in segment 2 of 4; truncation at each of the last 27
bytes; batches with empty and 10-byte streams between long ones.  Per stream, the cut list, the stop
and the size query's verdict and total equal a single lane's walk of the whole chain, and the
segments decoded alone by the oracle's Reader, joined, are the whole stream's output and error.
CPU only; the program exits non-zero at its first mismatch.

Also here: the route's C entry points are exported and refuse bad arguments without a device."""

import ctypes
import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_segs_parts.h", "ez_k2_segs.h", "ez_k2_walk.h")  # (ez_k2_walk.h: what emu_walk mirrors)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "cuts_found", "stops", "parts", "joined", "passed", "again", "again_adversarial", "again_entry", "again_marked",
           "walk_marked", "take_plain", "take_lead", "take_first", "stop_first", "filled", "fill_walked", "fill_skipped", "dead_parts",
           "seam_before", "seam_after", "packed40", "empty_straddle", "lead_not_cuts", "lead_all_cuts", "many_cuts", "lit_whole_part",
           "adversarial", "far_window_stop", "exact_window", "handover_then_resets", "err_seg2", "tail_cuts", "sized_ok", "sized_handed",
           "batch_streams", "batch_short", "batch_empty", "oracle_segments", "chunk256", "chunk1024")


def build_check(tmp):
    return k2_check_build.build_check("k2_segs_parts_check", tmp, HEADERS, opt="-O2")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("k2_segs_parts"))


def test_parts_steps_match_serial_walk_and_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["unsettled"] == 0  # (63 rounds repair any part: the counter is a bound, not a path)
    assert counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_before"] == 2 * 8 and counts["seam_after"] == 2  # both chunk sizes
    assert counts["empty_straddle"] == 2 * (5 + 8)  # 2 Resets at 5 offsets, 3 at 8
    assert counts["far_window_stop"] == counts["exact_window"] == counts["handover_then_resets"] == 2
    assert counts["stop_first"] >= 2  # (the stop that a record's first Reset brings, taken from the record)
    assert counts["again_entry"] + counts["again_marked"] == counts["again"] + counts["again_adversarial"]
    assert counts["tail_cuts"] % 27 == 0
    assert p.stdout.rstrip().endswith("ok")


def test_route_entry_points():
    import eazy_amd as ez

    lib = ez._lib()
    for n in ("ez_select_segments_route", "ez_segments_parts_last"):
        assert n in ez.exported_symbols() and hasattr(lib, n), n
    assert lib.ez_select_segments_route(ord("x")) == ez.EINVAL
    assert lib.ez_select_segments_route(ord("p")) == 0 and lib.ez_select_segments_route(ord("v")) == 0 and lib.ez_select_segments_route(0) == 0
    assert lib.ez_segments_parts_last(None) == ez.EINVAL
    c = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    st = lib.ez_segments_parts_last(c)
    assert st == (0 if ez.device_count() > 0 else ez.EDEVICE)
    if st != 0:
        assert list(c) == [0, 0, 0, 0]
