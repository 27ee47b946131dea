"""K2b's per-lane steps (eazy_amd/csrc/ez_k2_brk.h: kb_sum up to a chunk's first event, kb_walk with the
stream's state from there, the fill pass's second kb_sum with each lane's bases, over K2z's speculative
walk and its repair), compiled for the host by tools/k2_brk_check.hip and run over 64 emulated lanes as
the kernel runs them, for every chunk size, on hand-built streams: a Break at the last 8 positions
before a chunk seam and a super-block seam; a Break before any output, before the header's Reset, right
before and right after a Reset that follows output; 2, 3 and 5,000 Breaks back to back; Breaks around
padding runs and around Magic and Ver metas; literal bodies made of 80 1f, of 80 10 14 and of whole
headers (speculation starts inside them: the repair is counted); a 70,000-byte literal entered from
every lane with a Break after it; streams of 4 segments with Breaks in each; an error in the middle with
Breaks before and after it (bad magic, Ver 1, an unsupported meta, 80 18 xx, BlockSizeLimit, truncation
at each of the last 27 bytes, a lone trailing 0x80 among them).  Per stream, the chunked walk's verdict,
Break count, positions and total equal a single lane's walk of the whole chain (kb_serial), and a
stream the walk takes has exactly the oracle Reader's ErrBreak positions, size and clean end.
CPU only; the program exits non-zero at its first mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_brk.h", "ez_k2_segs.h", "ez_k2_walk.h")  # (ez_k2_walk.h: what emu_walk mirrors)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "breaks_found", "with_breaks", "taken", "stops", "seam_chunk", "seam_super", "first", "before_reset", "around_reset",
           "packed", "packed_chunk", "empty_message", "pad", "metas", "adversarial", "fix_rounds", "rewalks", "rewalks_adversarial",
           "lit_enter", "four_segments", "err_magic", "err_ver", "err_meta", "err_brklen", "err_limit", "trunc", "lone_80", "unlisted",
           "tail_cuts", "superblocks", "events", "chunk64", "chunk256", "chunk1024")


def build_check(tmp):
    """tools/k2_brk_check, built when it is missing or older than its sources."""
    return k2_check_build.build_check("k2_brk_check", tmp, HEADERS)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("k2_brk"))


def test_break_steps_match_serial_walk_and_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    # speculation that starts inside literal bodies made of Breaks, Resets and headers: the repair ran on those streams
    assert counts["rewalks_adversarial"] > 0
    assert counts["chunk64"] == counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_chunk"] == counts["seam_super"] == 3 * 8  # every chunk size, 8 positions
    assert counts["packed"] == 3 * 3 and counts["pad"] == 3 * 5
    assert counts["adversarial"] == 3 * (3 * 3 + 1)
    assert counts["lit_enter"] == 3 * 64  # from every lane
    assert counts["trunc"] == 27 and counts["lone_80"] == 1
    assert counts["err_magic"] == counts["err_ver"] == counts["err_meta"] == counts["err_brklen"] == counts["err_limit"] == 1
    assert counts["four_segments"] == 2 and counts["unlisted"] == 6
    assert p.stdout.rstrip().endswith("ok")
