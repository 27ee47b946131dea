"""K2g's per-lane steps (eazy_amd/csrc/ez_k2_segs.h: kg_sum up to a chunk's first event, kg_cuts with the
stream's state from there, over K2z's speculative walk and its repair), compiled for the host by
tools/k2_segs_check.hip and run over 64 emulated lanes as the kernel runs them, for every chunk size,
on hand-built streams: a late Reset at the last 8 positions before a chunk seam and a super-block
seam; 2, 3 and 40 Resets packed together, two with nothing between them, one straight after the
header's own, header-only streams; Magic, Ver and Break metas and padding runs around a cut; literal
bodies made of Resets and of whole headers (speculation starts inside them: the repair is counted); a
70,000-byte literal entered from every lane and followed by a Reset; segments with their own windows,
a distance only the other segment's window holds, copies that reach before their segment's start; an
error in segment 2 of 4 (bad magic, Ver 1, an unsupported meta, BlockSizeLimit, truncation at each of
the last 27 bytes).  Per stream, the cut list (input position, output position) and the stop equal a
single lane's walk of the whole chain, the number of cuts is the one the stream was built to have, and
each segment decoded alone by the oracle's Reader, joined, is the whole stream's output and error.
CPU only; the program exits non-zero at its first mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_segs.h", "ez_k2_walk.h")  # (ez_k2_walk.h: what emu_walk mirrors)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "cuts_found", "with_cuts", "stops", "stops_with_cuts", "seam_chunk", "seam_super", "packed", "packed_chunk",
           "empty_segment", "header_only", "metas_cut", "pad_cut", "break_cut", "adversarial", "fix_rounds", "rewalks",
           "rewalks_adversarial", "lit_enter", "windows", "overflow_stop", "zero_reach", "err_magic", "err_ver", "err_meta", "err_limit",
           "trunc_in_seg", "trunc_joined", "tail_cuts", "oracle_segments", "superblocks", "events", "chunk64", "chunk256", "chunk1024")


def build_check(tmp):
    """tools/k2_segs_check, built when it is missing or older than its sources."""
    return k2_check_build.build_check("k2_segs_check", tmp, HEADERS)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("k2_segs"))


def test_segment_steps_match_serial_walk_and_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    # speculation that starts inside literal bodies made of Resets and headers: the repair ran on those streams
    assert counts["rewalks_adversarial"] > 0
    assert counts["chunk64"] == counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_chunk"] == counts["seam_super"] == 3 * 8  # every chunk size, 8 positions
    assert counts["packed"] == 3 * 3 and counts["pad_cut"] == 3 * 5
    assert counts["lit_enter"] == 3 * 64  # from every lane
    assert counts["trunc_in_seg"] == counts["trunc_joined"] == 27
    assert counts["err_magic"] == counts["err_ver"] == counts["err_meta"] == 1 and counts["err_limit"] == 2
    assert counts["oracle_segments"] == counts["streams"] + counts["cuts_found"]  # every segment decoded alone
    assert p.stdout.rstrip().endswith("ok")
