"""The steps of K2b's parts route (eazy_amd/csrc/ez_k2_brk_parts.h: a lane's sum of its chunk of the
chain with its Breaks, the join of two sums in chain order, a part's record, the order pass that
follows the true chain through the records and leaves every part's entry state and the stream's
verdict, the fill from an entry state), compiled for the host by tools/k2_brk_parts_check.hip and run
over emulated lanes, parts and streams exactly as the kernels order them, for chunk 256 and chunk
1,024, on hand-built streams of 2 to 6 parts: a Break at each of the last 8 positions before a part
seam and at the first after it (the 80 a part's last byte, the 1f in the next part); 5,000 Breaks back
to back across a seam; 2 and 3 Breaks straddling a seam at every offset; a Break before the stream's
first output byte; a part whose only Breaks lie behind a Reset; a Break right before and right after a
Reset at a seam; a literal of 80 1f over exactly one whole part (passed through, counts nothing);
literal bodies of 80 1f, 80 10 14, whole headers and copy headers across seams (parts walked again:
counted); a segment over three parts with a distance past its window and a hand-over form in a late
part, each with Breaks in earlier parts (the whole stream handed over); an error in the middle with
Breaks on both sides; truncation at each of the last 27 bytes; batches with empty and 10-byte streams
between long ones.  Per stream, the verdict, count, total and every position equal a single lane's
walk of the whole chain, every position is stored exactly once, only the parts that hold a Break are
staged by the fill, and a stream the route takes has the oracle Reader's ErrBreak positions, size and
clean end.  CPU only; the program exits non-zero at its first mismatch.

Also here: the route's C entry points are exported and refuse bad arguments without a device."""

import ctypes
import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_brk_parts.h", "ez_k2_brk.h", "ez_k2_segs_parts.h", "ez_k2_segs.h", "ez_k2_walk.h",
                                                      "ez_k2_brk_walk.h")  # (the last two: what emu_walk and emu_block mirror)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "breaks_found", "taken", "stops", "parts", "joined", "passed", "again", "again_adversarial", "again_entry", "again_marked",
           "walk_marked", "filled", "fill_skipped", "fill_handed", "dead_parts", "seam_before", "seam_after", "many_breaks", "straddle",
           "first_output", "behind_reset", "around_reset_seam", "spanned", "adversarial", "far_window_stop", "handover_late", "err_mid",
           "tail_cuts", "batch_streams", "batch_short", "batch_empty", "chunk256", "chunk1024")


def build_check(tmp):
    return k2_check_build.build_check("k2_brk_parts_check", tmp, HEADERS, opt="-O2")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("k2_brk_parts"))


def test_parts_steps_match_serial_walk_and_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["unsettled"] == 0  # (63 rounds repair any part: the counter is a bound, not a path)
    assert counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_before"] == 2 * 8 and counts["seam_after"] == 2  # both chunk sizes
    assert counts["straddle"] == 2 * (3 + 5)  # 2 Breaks at 3 offsets, 3 at 5
    assert counts["many_breaks"] == counts["spanned"] == counts["far_window_stop"] == counts["handover_late"] == 2
    assert counts["err_mid"] == 2 * 5 and counts["tail_cuts"] == 2 * 2 * 27
    assert counts["again_entry"] + counts["again_marked"] == counts["again"] + counts["again_adversarial"]
    assert counts["breaks_found"] > 10000
    assert p.stdout.rstrip().endswith("ok")


def test_route_entry_points():
    import eazy_amd as ez

    lib = ez._lib()
    for n in ("ez_select_breaks_route", "ez_breaks_parts_last"):
        assert n in ez.exported_symbols() and hasattr(lib, n), n
    assert lib.ez_select_breaks_route(ord("x")) == ez.EINVAL
    assert lib.ez_select_breaks_route(ord("p")) == 0 and lib.ez_select_breaks_route(ord("v")) == 0 and lib.ez_select_breaks_route(0) == 0
    assert lib.ez_breaks_parts_last(None) == ez.EINVAL
    c = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    st = lib.ez_breaks_parts_last(c)
    assert st == (0 if ez.device_count() > 0 else ez.EDEVICE)
    if st != 0:
        assert list(c) == [0, 0, 0, 0]
    assert callable(ez.select_breaks_route) and callable(ez.breaks_parts_last)
