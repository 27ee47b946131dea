#!/usr/bin/env python3
"""Wall time of one 100-byte log line on each of N live Writer handles: one ez_writer_write_many
call against the same Writes as N ez_writer_write calls in the same process (the only route for
this shape without the call, so the baseline).  Median of 20 calls after 3 warm-ups, N = 64 and
1,024, block 1 MiB / table 1,024 and block 64 KiB / table 1,024.

    python tools/perf_write_many.py [--out profiles/write_many.json] [--commit HASH]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, CALLS, LINE = 3, 20, 100
VP = C.c_void_p


def lines(seed, count):
    rng = np.random.default_rng(seed)
    words = [b"GET", b"POST", b"/api/v1/items", b"/index.html", b"status=200", b"status=404", b"user=", b"latency_ms=", b"conn", b"tenant-", b"INFO", b"WARN"]
    out = []
    for _ in range(count):
        b = b"2026-01-01T00:00:%02d " % int(rng.integers(0, 60))
        while len(b) < LINE:
            b += words[int(rng.integers(0, len(words)))] + b"%d " % int(rng.integers(0, 100000))
        out.append(b[:LINE])
    return out


def measure(ez, L, n, block, htable):
    def handles():
        hs = []
        for _ in range(n):
            h = VP()
            assert L.ez_writer_new(block, htable, 0, C.byref(h)) == 0
            hs.append(h)
        return hs

    many, single = handles(), handles()
    arr = (VP * n)(*[h.value for h in many])
    bound = ez.compress_bound(LINE)
    ends = np.arange(1, n + 1, dtype=np.uint64) * LINE
    out = np.zeros(n * bound + 64, np.uint8)
    oe = np.zeros(n, np.uint64)
    st = np.zeros(n, np.int32)
    got = C.c_size_t()
    t_many, t_single, same = [], [], True
    for it in range(WARM + CALLS):
        ls = lines(100 * n + it, n)
        src = np.frombuffer(b"".join(ls), np.uint8).copy()
        t0 = time.perf_counter()
        rc = L.ez_writer_write_many(arr, n, VP(src.ctypes.data), VP(ends.ctypes.data), VP(out.ctypes.data), n * bound,
                                    VP(oe.ctypes.data), VP(st.ctypes.data))
        t1 = time.perf_counter()
        assert rc == 0, rc
        route = ez.compress_route_last()
        a = out[: int(oe[-1])].tobytes()
        one = np.zeros(bound + 64, np.uint8)
        parts = []
        t2 = time.perf_counter()
        for j in range(n):
            rc = L.ez_writer_write(single[j], VP(src.ctypes.data + j * LINE), LINE, VP(one.ctypes.data), bound, C.byref(got))
            parts.append(one[: got.value].tobytes())
        t3 = time.perf_counter()
        assert rc == 0, rc
        same = same and a == b"".join(parts)
        if it >= WARM:
            t_many.append((t1 - t0) * 1e6)
            t_single.append((t3 - t2) * 1e6)
    for h in many + single:
        L.ez_writer_free(h)
    m, s = statistics.median(t_many), statistics.median(t_single)
    return {
        "handles": n, "block": block, "htable": htable, "line_bytes": LINE, "route": route, "same_bytes": same,
        "write_many_us_per_call": round(m, 1), "write_many_us_per_write": round(m / n, 3),
        "single_writes_us_per_round": round(s, 1), "single_writes_us_per_write": round(s / n, 3),
        "speedup": round(s / m, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_many.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as the tests load it)

    import eazy_amd as ez

    L = ez._lib()
    L.ez_writer_write_many.argtypes = [VP, C.c_size_t, VP, VP, VP, C.c_size_t, VP, VP]
    L.ez_writer_write.argtypes = [VP, VP, C.c_size_t, VP, C.c_size_t, C.POINTER(C.c_size_t)]
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() or "unknown"
    rows = [measure(ez, L, n, block, htable) for block, htable in ((1 << 20, 1024), (1 << 16, 1024)) for n in (64, 1024)]
    res = {"commit": commit, "warmups": WARM, "calls": CALLS, "statistic": "median wall time, microseconds", "rows": rows}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
