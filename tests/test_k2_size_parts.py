"""The steps of K2z's parts route (eazy_amd/csrc/ez_k2_parts.h with ez_k2_size.h's: the speculative
walk of a part with a warm-up chunk before it, verify, repair and sum, the part's record, and the
in-order pass that follows the true chain through the records), compiled for the host by
tools/k2_size_parts_check.hip and run over emulated lanes, parts and streams exactly as the kernels
order them, for chunk 256 and chunk 1,024, on hand-built streams: every header form at the last 8
positions before a part seam; a literal from every lane that ends within a part's length, spans
exactly one whole part, spans three whole parts; literal bodies that parse as copy headers across part
seams (parts walked again: counted); a literal body of wide metas over a whole part (the part's record
is bad, the stream is taken); padding runs across part seams; a MetaReset after output in a later
part; every stream cut at each of its last 27 bytes; a batch with empty and very short streams between
long ones; the automatic route's probe on every stream, both answers counted.  Per stream, (size, taken or handed over) equals the oracle's Reader and a single lane's
walk of the whole chain.  CPU only; the program exits non-zero at its first mismatch.

Also here: the route's C entry points are exported and refuse bad arguments without a device."""

import ctypes
import re
import subprocess

import pytest

import k2_check_build

HEADERS = k2_check_build.COMMON + k2_check_build.csrc("ez_k2_walk.h")  # (ez_k2_walk.h: what emu_walk mirrors)

# the classes the program counts: each must have been visited
CLASSES = ("streams", "taken", "handed_error", "handed_design", "seam_part", "lit_within", "lit_one_part", "lit_many_parts", "adversarial",
           "parts", "joined", "passed", "walked", "walked_adversarial", "garbage_bad", "garbage_bad_taken", "pad_seam", "reset_late_part",
           "cuts", "cuts_taken", "cuts_handed_ok", "batch_streams", "batch_short", "batch_parts", "probe_wave", "probe_parts", "chunk256", "chunk1024")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return k2_check_build.build_check("k2_size_parts_check", tmp_path_factory.mktemp("k2_size_parts"), HEADERS, opt="-O2")


def test_parts_steps_match_oracle(check):
    p = subprocess.run([check], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w+)\s+(\d+)$", p.stdout, re.M)}
    for c in CLASSES:
        assert counts.get(c, 0) > 0, f"class {c} never visited: {counts}"
    assert counts["unsettled"] == 0  # (63 rounds repair any part: the counter is a bound, not a path)
    assert counts["chunk256"] == counts["chunk1024"] == counts["streams"]
    assert counts["seam_part"] == 2 * 21 * 8  # both chunk sizes, every form, 8 positions
    assert counts["lit_within"] == counts["lit_one_part"] == counts["lit_many_parts"] == 2 * 64  # from every lane
    assert counts["pad_seam"] == 2 * 40 * 3
    assert counts["cuts"] >= 27 * (counts["streams"] - counts["cuts"]) - 27 * 4  # (the shortest streams have fewer bytes)
    assert p.stdout.rstrip().endswith("ok")


def test_route_entry_points():
    import eazy_amd as ez

    lib = ez._lib()
    for n in ("ez_select_size_route", "ez_decompressed_size_parts_last"):
        assert n in ez.exported_symbols() and hasattr(lib, n), n
    assert lib.ez_select_size_route(ord("x")) == ez.EINVAL
    assert lib.ez_select_size_route(ord("p")) == 0 and lib.ez_select_size_route(ord("v")) == 0 and lib.ez_select_size_route(0) == 0
    assert lib.ez_decompressed_size_parts_last(None) == ez.EINVAL
    c = (ctypes.c_uint64 * 3)(7, 7, 7)
    st = lib.ez_decompressed_size_parts_last(c)
    assert st == (0 if ez.device_count() > 0 else ez.EDEVICE)
    if st != 0:
        assert list(c) == [0, 0, 0]
