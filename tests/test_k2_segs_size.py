"""The size query's K2g stage (k2g_size, eazy_amd/csrc/ez_decompress_segs.hip: K2g's walk behind K2z's
kernels, which sizes concatenated streams and hands the others on to the exact decoder), its per-lane
steps and its end step (ez_k2_segs.h: kg_sum, kg_cuts, kg_end_ok) compiled for the host by
tools/k2_segs_size_check.hip and run over 64 emulated lanes as the kernel runs them, for every chunk
size, on the streams tools/k2_segs_check --dump writes (Resets at chunk and super-block seams, packed
Resets, literal bodies made of Resets and headers, the 70,000-byte literal, a window per segment,
errors in segment 2 of 4), on one of them with several cuts truncated at each of its last 27 bytes, and
on four streams whose last segment fails the end check.  Per stream the verdict (sized, or handed on)
and the total equal a single walker's; a sized stream's total is the oracle Reader's output length
read to EOF, without an error; every dumped stream with a cut, no stop and no error is sized.
CPU only; the program exits non-zero at its first mismatch and prints the stream."""

import re
import subprocess

import pytest

import k2_check_build
from test_k2_segments import HEADERS, build_check as build_segs_check

# the classes the program counts: each must have been visited
CLASSES = ("streams", "dumped", "sized", "sized_with_cuts", "handed_stop", "handed_end", "truncations", "truncations_sized", "own",
           "must_size", "superblocks", "events", "chunk64", "chunk256", "chunk1024")


def build_check(tmp):
    """tools/k2_segs_size_check, built when it is missing or older than its sources."""
    return k2_check_build.build_check("k2_segs_size_check", tmp, HEADERS)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("k2_segs_size")
    dump = tmp / "streams.bin"
    p = subprocess.run([build_segs_check(tmp), "--dump", str(dump)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return subprocess.run([build_check(tmp), str(dump)], capture_output=True, text=True, timeout=600)


def test_size_stage_matches_serial_walk_and_oracle(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", run.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["dumped"] > 300 and counts["streams"] == counts["dumped"] + 27 + 4
    assert counts["truncations"] == 27 and counts["own"] == 4
    assert counts["truncations_sized"] < 27  # (a cut inside a token is handed on, one between tokens is sized)
    assert counts["sized"] + counts["handed_stop"] + counts["handed_end"] == counts["streams"]
    assert counts["handed_end"] >= counts["own"]
    # every dumped stream with a cut and no stop that the oracle decodes without an error was sized
    assert 0 < counts["must_size"] <= counts["sized_with_cuts"]
    assert counts["chunk64"] == counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert run.stdout.rstrip().endswith("ok")
