"""The part layout of the K2 parts routes (eazy_amd/csrc/ez_k2_layout.h: layout_range, layout_gate,
layout_scan, parts_cap, the steps of kp_layout) held on the host to a serial layout by
tools/k2_layout_check.cpp, a stand-alone program built with the host compiler under AddressSanitizer
and UndefinedBehaviorSanitizer.  No GPU, nothing preloaded."""

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases the program must have run, from its enumeration and not from its output, per part size
# (16,384 and 65,536 bytes):
#   a batch runs under 8 settings: 5 hints (exact, one less, 0, 1, four times), descending offsets, and
#   two caps under the exact hint (the batch's parts, one fewer)
#   T = 8: 9 counts (0, 1, 2, 7, 8, 9, 16, 17, 23) x 8 rotations of the 8 stream lengths: 72 batches
#   T = 1,024: 2 counts (1,025 and 2,049), one rotation: 2 batches
#   parts_cap: 4 sums around 2^31, each from the bytes and from the streams: 8; 4 at the ends of 64 bits
CASES = 2 * ((9 * 8 + 2) * 8 + 4 * 2 + 4)
assert CASES == 1208


def test_layout_steps_equal_the_serial_layout(tmp_path):
    exe = str(tmp_path / "k2_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # (the runtimes in the program itself: no order among loaded libraries matters)
           "-I", os.path.join(ROOT, "eazy_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "k2_layout_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"k2_layout ok: (\d+) cases", p.stdout)
    assert m and int(m.group(1)) == CASES, p.stdout[-500:]
