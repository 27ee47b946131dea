"""K2j's steps (eazy_amd/csrc/ez_k2_jump.h: the chunk view, the speculative walk, the follow walk, the
token walk, the stream's checks, kj_piece), compiled for the host by tools/k2_jump_check.hip and run
stage by stage as the kernels run them, over K2j's own workspace layout and a staging buffer of the
kernels' size, on hand-built streams at both chunk sizes: every header form at each position before a
chunk seam, a 70,000-byte literal, the off-phase stream whose speculation never merges (repairs
counted), literal bodies that parse as tokens, padding across seams and at a stream's end, invalid
streams, batch shapes, and every stream cut at each of its last 27 bytes, as a batch stream and as a
continuation.  Per stream, the bytes and the size equal the oracle's Reader, the verdict and a
continuation's stop equal one in-order walk.  CPU only; the program exits non-zero at its first
mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_jump.h", "ez_internal.h")

# the classes the program counts: each must have been visited
CLASSES = ("runs", "streams", "taken", "handed_error", "handed_design", "jc256", "jc1024", "blocks", "seams", "lit_enter", "passthrough",
           "merged", "repairs", "phase_repairs", "bodies", "pad_seam", "pad_tail", "cuts", "cuts_taken", "cuts_handed_ok", "c_on", "stops",
           "tails", "multi", "empty", "one_chunk", "late_reset", "no_reset", "far_distance", "short_slot", "breaks")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return k2_check_build.build_check("k2_jump_check", tmp_path_factory.mktemp("k2_jump"), HEADERS)


def test_jump_steps_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["jc256"] + counts["jc1024"] == counts["runs"]
    assert counts["seams"] == 2 * sum(min(n, 16) + 1 for n in FORM_BYTES)  # both chunk sizes, every form, every position
    assert counts["taken"] + counts["handed_error"] + counts["handed_design"] + counts["cuts_handed_ok"] == counts["streams"]
    assert p.stdout.rstrip().endswith("ok")


# the byte lengths of tools/k2_check_common.h forms(), in its order
FORM_BYTES = (51, 202, 1003, 70005, 2, 3, 4, 4, 5, 6, 7, 3, 2, 2, 3, 6, 1, 15, 16, 17, 40)
