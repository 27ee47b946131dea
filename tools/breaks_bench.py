"""K2b against the size query: the time of the batch Break index (ez_stream_breaks_batch), of
ez_decompressed_size_batch on the same batch (the same bytes walked once) and of the Break index
without a workspace (the exact decoder alone: what a caller had to pay before).

    python tools/breaks_bench.py [--streams 4096] [--stream-bytes 65536] [--every 512] [--runs 20] [--out FILE]

Two batches of log streams written by the oracle's Writer: one with a Break every ~`every` bytes of
text, and the same text without any Break.  Each call is timed with device events, alternating the
three calls in one loop after a warm-up; the median of the runs is reported with the 10th and 90th
percentiles as the run-to-run spread.  The query's arrays are checked first: with and without a
workspace they are equal, the sizes are the stream lengths, and the Break counts are the ones
written.  One JSON line per batch, with the hash of the kernel sources.  Needs a GPU; there is no
fallback."""

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SOURCES = ("ez_decompress_brk.hip", "ez_k2_brk.h", "ez_k2_segs.h", "ez_k2_size.h", "ez_k2_walk.h", "ez_k2_parse.h", "ez_decompress.hip",
           "ez_decompress_size.hip", "ez_decompress_segs.hip")


def source_hash():
    h = hashlib.sha256()
    for n in SOURCES:
        h.update(open(os.path.join(ROOT, "eazy_amd", "csrc", n), "rb").read())
    return h.hexdigest()[:16]


def log_lines(rng, n):
    out = bytearray()
    while len(out) < n:
        out += b"2026-01-01T00:00:%02d INFO tenant-%d GET /api/v1/items/%d status=200 bytes=%d\n" % (
            rng.integers(60), rng.integers(13), rng.integers(5000), rng.integers(100000))
    return bytes(out[:n])


def build_batches(streams, stream_bytes, every, distinct):
    """`distinct` different streams by the oracle's Writer, repeated to `streams` -> {name: (streams, Breaks per stream)}."""
    import numpy as np

    import oracle as orc

    rng = np.random.default_rng(41)
    with_brk, without, counts = [], [], []
    for _ in range(distinct):
        text = log_lines(rng, stream_bytes)
        wb, wn = orc.Writer(1 << 20, 1024), orc.Writer(1 << 20, 1024)
        at, n = 0, 0
        while at < len(text):
            m = text[at : at + every - 32 + int(rng.integers(64))]
            assert wb.write(m) == (len(m), 0) and wn.write(m) == (len(m), 0)
            assert wb.write_break() == 0
            at += len(m)
            n += 1
        with_brk.append(wb.sink)
        without.append(wn.sink)
        counts.append(n)
    rep = lambda v: [v[k % distinct] for k in range(streams)]  # noqa: E731
    return {"breaks": (rep(with_brk), rep(counts)), "no_breaks": (rep(without), [0] * streams)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--every", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64, help="different streams the host writes; the batch repeats them")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import eazy_amd as ez

    if not torch.cuda.is_available():
        raise SystemExit("breaks_bench: no GPU")
    dev = torch.device("cuda:0")
    L = ez._lib()
    import ctypes as C

    def timed(fn):  # (one run: `inner` calls back to back between two events, so that the window is not the events' own)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    for name, (ins, counts) in build_batches(args.streams, args.stream_bytes, args.every, min(args.distinct, args.streams)).items():
        count = len(ins)
        coff = np.concatenate([[0], np.cumsum([len(b) for b in ins])]).astype(np.int64)
        comp = torch.from_numpy(np.frombuffer(b"".join(ins) + b"\0" * 16, np.uint8).copy()).to(dev)
        d_coff = torch.from_numpy(coff).to(dev)
        max_in = max(len(b) for b in ins)
        found = sum(counts)
        sizes = torch.empty(count, dtype=torch.int64, device=dev)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        brk_idx = torch.empty(count + 1, dtype=torch.int64, device=dev)
        brk_pos = torch.empty(found + 1, dtype=torch.int64, device=dev)
        brk_total = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(L.ez_breaks_workspace(count), dtype=torch.uint8, device=dev)
        zws = torch.empty(L.ez_decompress_workspace(count), dtype=torch.uint8, device=dev)
        b = ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, None, sizes.data_ptr(), status.data_ptr(), count, max_in, 0, 0)
        sp = ez._stream_ptr(None)

        def breaks(workspace):
            def call():
                st = L.ez_stream_breaks_batch(0, C.byref(b), brk_idx.data_ptr(), brk_pos.data_ptr(), found + 1, brk_total.data_ptr(), workspace, sp)
                assert st == ez.OK, st
            return call

        def size_query():
            st = L.ez_decompressed_size_batch(0, C.byref(b), zws.data_ptr(), sp)
            assert st == ez.OK, st

        legs = {"breaks": breaks(ws.data_ptr()), "size_query": size_query, "breaks_exact_only": breaks(None)}
        got = {}
        for k, fn in legs.items():  # results first
            sizes.fill_(-1)
            brk_pos.fill_(-1)
            fn()
            torch.cuda.synchronize()
            assert sizes.cpu().numpy().tolist() == [args.stream_bytes] * count and int(status.abs().sum()) == 0, (name, k)
            if k != "size_query":
                got[k] = (brk_idx.cpu().numpy().copy(), brk_pos.cpu().numpy().copy(), tuple(brk_total.cpu().numpy()))
                assert got[k][2] == (found, found) and np.diff(got[k][0]).tolist() == counts, (name, k)
        assert all(np.array_equal(x, y) for x, y in zip(got["breaks"][:2], got["breaks_exact_only"][:2])), name
        handed = int(ws[60:64].cpu().numpy().view(np.uint32)[0])  # (the workspace's hand-over list: its length)
        for fn in legs.values():
            for _ in range(args.warmup):
                timed(fn)
        times = {k: [] for k in legs}
        for _ in range(args.runs):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        res = {"batch": name, "streams": count, "stream_bytes": args.stream_bytes, "compressed_bytes": int(coff[-1]),
               "longest_compressed_stream": max_in, "breaks_found": found, "handed_to_exact": handed, "chunk": ez.decompressed_size_chunk(max_in),
               "size_query_route": ez.decompressed_size_chunk_last(), "runs": args.runs, "calls_per_run": args.inner, "device": torch.cuda.get_device_name(0),
               "kernel_source_sha256_16": source_hash()}
        for k, v in times.items():
            v = np.array(v)
            res[k] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                      "p90_ms": round(float(np.percentile(v, 90)), 4)}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del comp


if __name__ == "__main__":
    main()
