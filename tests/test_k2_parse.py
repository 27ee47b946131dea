"""The parse primitives the batch decoders share (eazy_amd/csrc/ez_k2_parse.h: k2_scan, fast_tok and
K2j's speculative step jadv_fast), compiled for the host by tools/k2_parse_check.hip and compared
header by header with the oracle's Decoder and the steps its Reader takes: every value of a header's
first three bytes, edge values in the next five, zero runs, the metas, and the input cut at every
point inside a header.  CPU only; the program exits non-zero at its first mismatch and prints the
header."""

import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON

# the classes the program counts: each must have been visited
CLASSES = ("headers", "pad", "skip", "reset", "lit", "copy", "zero_region", "rejected", "handed_wide_meta", "handed_big", "fast",
           "part_cuts", "part_pad", "part_token", "tail_header", "tail_literal", "tail_rejected",
           "m_break", "m_reset_ok", "m_reset_bad", "m_ver_ok", "m_ver_bad", "m_magic_ok", "m_magic_bad", "m_wide", "m_unknown")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return k2_check_build.build_check("k2_parse_check", tmp_path_factory.mktemp("k2_parse"), HEADERS)


def test_parse_primitives_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["headers"] >= 1 << 24  # every value of bytes 0..2
    assert p.stdout.rstrip().endswith("ok")
