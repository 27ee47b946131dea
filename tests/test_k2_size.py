"""K2z's per-lane steps (eazy_amd/csrc/ez_k2_size.h: the speculative walk, the verify walk and its
repair, the sum walk, the end checks), compiled for the host by tools/k2_size_check.hip and run over
64 emulated lanes exactly as the kernel runs them, for every chunk size, on hand-built streams: every
header form at the last 8 positions before a chunk seam and before a super-block seam, a 70,000-byte
literal entered from every lane, literal bodies that parse as copy headers (speculation off the true
chain for whole chunks: the re-walks are counted), padding runs across seams and at the end, and
every stream cut at each of its last 27 bytes.  Per stream, (size, taken or handed over) equals the
oracle's Reader and a single lane's walk of the whole chain.  CPU only; the program exits non-zero at
its first mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_walk.h")  # (ez_k2_walk.h: what emu_walk mirrors)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "taken", "handed_error", "handed_design", "seam_chunk", "seam_super", "lit_enter", "lit_skip", "adversarial",
           "fix_rounds", "rewalks", "rewalks_adversarial", "pad_seam", "pad_tail", "cuts", "cuts_taken", "cuts_handed_ok",
           "superblocks", "passthrough", "merged", "chunk64", "chunk256", "chunk1024")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return k2_check_build.build_check("k2_size_check", tmp_path_factory.mktemp("k2_size"), HEADERS)


def test_size_steps_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    # speculation kept off the true chain: the repair ran on those streams
    assert counts["rewalks_adversarial"] > 0
    assert counts["chunk64"] == counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_chunk"] == counts["seam_super"] == 3 * 21 * 8  # every chunk size, every form, 8 positions
    assert counts["lit_enter"] == 3 * 64  # from every lane
    assert counts["cuts"] >= 27 * (counts["streams"] - counts["cuts"]) - 27 * 4  # (the shortest streams have fewer bytes)
    assert p.stdout.rstrip().endswith("ok")
