"""K2z's per-lane steps (eazy_amd/csrc/ez_k2_size.h: the speculative walk, the verify walk and its
repair, the sum walk, the end checks), compiled for the host by tools/k2_size_check.hip and run over
64 emulated lanes exactly as the kernel runs them, for every chunk size, on hand-built streams: every
header form at the last 8 positions before a chunk seam and before a super-block seam, a 70,000-byte
literal entered from every lane, literal bodies that parse as copy headers (speculation off the true
chain for whole chunks: the re-walks are counted), padding runs across seams and at the end, and
every stream cut at each of its last 27 bytes.  Per stream, (size, taken or handed over) equals the
oracle's Reader and a single lane's walk of the whole chain.  CPU only; the program exits non-zero at
its first mismatch and prints the stream."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "k2_size_check")

# the classes the program counts: each must have been visited
CLASSES = ("streams", "taken", "handed_error", "handed_design", "seam_chunk", "seam_super", "lit_enter", "lit_skip", "adversarial",
           "fix_rounds", "rewalks", "rewalks_adversarial", "pad_seam", "pad_tail", "cuts", "cuts_taken", "cuts_handed_ok",
           "superblocks", "passthrough", "merged", "chunk64", "chunk256", "chunk1024")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    src = os.path.join(ROOT, "tools", "k2_size_check.hip")
    orc_c = os.path.join(ROOT, "oracle", "eazy_oracle.c")
    deps = [src, orc_c, os.path.join(ROOT, "oracle", "eazy_oracle.h"), os.path.join(ROOT, "include", "eazy.h")]
    deps += [os.path.join(ROOT, "eazy_amd", "csrc", f) for f in ("ez_k2_size.h", "ez_k2_parse.h", "ez_bytes.h", "ez_format.h")]
    if not os.path.exists(CHECK) or os.path.getmtime(CHECK) < max(os.path.getmtime(d) for d in deps):
        tmp = tmp_path_factory.mktemp("k2_size")
        orc_o, chk_o = str(tmp / "eazy_oracle.o"), str(tmp / "k2_size_check.o")
        hipcc = "/opt/rocm/bin/hipcc"
        for cmd in (["gcc", "-O2", "-std=c11", "-c", "-o", orc_o, orc_c],
                    [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-align-mismatch", "-c", "-o", chk_o, src],
                    [hipcc, "-o", CHECK, chk_o, orc_o, "-lpthread"]):
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
    return CHECK


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
