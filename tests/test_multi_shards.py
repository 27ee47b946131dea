"""The shard arithmetic of the multi-device batch calls (eazy_amd/csrc/ez_multi_shards.h: shard_bounds,
rebased, max_span, offsets_ascend) held on the host to a brute-force statement of its rule by
tools/multi_shards_check.cpp, a stand-alone program built with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU, nothing preloaded."""

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cases the program must have run, from its enumeration and not from its output:
#   length vectors over {0, 1, 2, 5} with count 0..6: 4^0 + ... + 4^6 = 5461, each on nshard 1..9 and
#   off[0] in {0, 7}: 5461 * 9 * 2 = 98298
#   one stream of 1000 among 60 of 1 at three places, nshard 1..9: 27
#   20 empty streams, nshard 1..9, off[0] in {0, 7}: 18
#   1, 2 and 3 streams on 4..9 shards: 18
#   four totals past 32 and 63 bits in three streams, nshard 1..9, off[0] in {0, 7}: 72
CASES = 5461 * 9 * 2 + 3 * 9 + 9 * 2 + 3 * 6 + 4 * 9 * 2
assert CASES == 98433


def test_shard_arithmetic_equals_the_brute_force_rule(tmp_path):
    exe = str(tmp_path / "multi_shards_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # (the runtimes in the program itself: no order among loaded libraries matters)
           "-I", os.path.join(ROOT, "eazy_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "multi_shards_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"multi_shards ok: (\d+) cases", p.stdout)
    assert m and int(m.group(1)) == CASES, p.stdout[-500:]
