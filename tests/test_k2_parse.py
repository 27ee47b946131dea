"""The parse primitives the batch decoders share (eazy_amd/csrc/ez_k2_parse.h: k2_scan, fast_tok and
K2j's speculative step jadv_fast), compiled for the host by tools/k2_parse_check.hip and compared
header by header with the oracle's Decoder and the steps its Reader takes: every value of a header's
first three bytes, edge values in the next five, zero runs, the metas, and the input cut at every
point inside a header.  CPU only; the program exits non-zero at its first mismatch and prints the
header."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "k2_parse_check")

# the classes the program counts: each must have been visited
CLASSES = ("headers", "pad", "skip", "reset", "lit", "copy", "zero_region", "rejected", "handed_wide_meta", "handed_big", "fast",
           "part_cuts", "part_pad", "part_token", "tail_header", "tail_literal", "tail_rejected",
           "m_break", "m_reset_ok", "m_reset_bad", "m_ver_ok", "m_ver_bad", "m_magic_ok", "m_magic_bad", "m_wide", "m_unknown")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    src = os.path.join(ROOT, "tools", "k2_parse_check.hip")
    orc_c = os.path.join(ROOT, "oracle", "eazy_oracle.c")
    deps = [src, orc_c, os.path.join(ROOT, "oracle", "eazy_oracle.h"), os.path.join(ROOT, "include", "eazy.h")]
    deps += [os.path.join(ROOT, "eazy_amd", "csrc", f) for f in ("ez_k2_parse.h", "ez_bytes.h", "ez_format.h")]
    if not os.path.exists(CHECK) or os.path.getmtime(CHECK) < max(os.path.getmtime(d) for d in deps):
        tmp = tmp_path_factory.mktemp("k2_parse")
        orc_o, chk_o = str(tmp / "eazy_oracle.o"), str(tmp / "k2_parse_check.o")
        hipcc = "/opt/rocm/bin/hipcc"
        for cmd in (["gcc", "-O2", "-std=c11", "-c", "-o", orc_o, orc_c],
                    [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-align-mismatch", "-c", "-o", chk_o, src],
                    [hipcc, "-o", CHECK, chk_o, orc_o, "-lpthread"]):
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
    return CHECK


def test_parse_primitives_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["headers"] >= 1 << 24  # every value of bytes 0..2
    assert p.stdout.rstrip().endswith("ok")
