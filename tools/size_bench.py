"""K2z against the full decode: the time of the batch decoded-size query (ez_decompressed_size_batch)
and, in the same process, of decompress_batch with its hints, on bench.py's workloads (its own
generators: c1 65,536 x 4 KiB and c2 4,096 x 256 KiB logs, c4 and c4s 64 x 4 MiB gradient buckets).

    python tools/size_bench.py [--workloads c1,c2,c4,c4s] [--rounds 15] [--out FILE]

Per workload the batch is compressed on the device (compress_batch + pack) and then, alternating in
one loop after a warm-up, timed with device events: the query under the hint a caller would give (the
longest compressed stream), the query under the hints 4096 (the small chunk, or from 4,096 streams
on the lane-per-stream kernel: "chunk" 1), 0 (the middle chunk) and 1 MiB (the large chunk), the
exact decoder alone run dry, and the decode.  Each timed window repeats its call until it lasts
about 20 ms.  The query's sizes are checked against the stream lengths.  One
JSON line per workload: medians in ms, the 10th and 90th percentiles as the run-to-run spread, and
whether the query's p90 lies below the decode's p10.  Needs a GPU; there is no fallback."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c1,c2,c4,c4s")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import eazy_amd as ez
    from eazy_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("size_bench: no GPU")
    dev = torch.device("cuda:0")

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    for name in args.workloads.split(","):
        count, size, block, htable, desc = bench.WORKLOADS[name]
        host, _ = bench.workload_bytes(name, 1, count * size)
        offs = synth.batch_offsets(count, size)
        data = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        off = torch.from_numpy(offs).to(dev)
        cb = ez.compress_batch(data, off, block, htable, max_len=size)
        packed, poff = ez.pack(cb)
        torch.cuda.synchronize()
        assert int(cb.status.abs().sum()) == 0
        del cb
        comp_len = (poff[1:] - poff[:-1])
        max_in, in_bytes = int(comp_len.max().item()), int((poff[-1] - poff[0]).item())
        out = torch.empty(count * size + 16, dtype=torch.uint8, device=dev)
        dsz = torch.empty(count, dtype=torch.int64, device=dev)
        dst = torch.empty(count, dtype=torch.int32, device=dev)
        qsz = torch.empty(count, dtype=torch.int64, device=dev)
        qst = torch.empty(count, dtype=torch.int32, device=dev)
        ws = torch.empty(ez._lib().ez_decompress_workspace(count), dtype=torch.uint8, device=dev)

        def query(hint, exact=False):
            return lambda: ez.decompressed_sizes(packed, poff, sizes=qsz, status=qst, workspace=ws, exact_only=exact, max_len=hint)

        def decode():
            ez.decompress_batch(packed, poff, off, out=out, sizes=dsz, status=dst, workspace=ws, max_len=size, in_bytes=in_bytes,
                                out_bytes=count * size)

        legs = {"query": query(max_in), "query_hint4096": query(4096), "query_hint0": query(0), "query_hint1m": query(1 << 20),
                "query_exact": query(0, True), "decode": decode}
        chunks, handed = {}, {}
        for k, fn in legs.items():  # results first: every leg reports the stream lengths
            qsz.fill_(-1)
            fn()
            torch.cuda.synchronize()
            if k != "decode":
                chunks[k] = ez.decompressed_size_chunk_last()
                handed[k] = int(ws[:4].cpu().numpy().view(np.uint32)[0]) if k != "query_exact" else count
                assert qsz.cpu().numpy().tolist() == [size] * count and int(qst.abs().sum()) == 0, (name, k)
            else:
                assert dsz.cpu().numpy().tolist() == [size] * count and int(dst.abs().sum()) == 0, name
                assert torch.equal(out[: count * size], data), name
        inner = {}
        for k, fn in legs.items():
            for _ in range(args.warmup):
                t = timed(fn, 1)
            inner[k] = max(1, min(200, int(args.window_ms / max(t, 1e-3))))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, inner[k]))
        res = {"workload": name, "desc": desc, "streams": count, "stream_bytes": size, "compressed_bytes": in_bytes,
               "longest_compressed_stream": max_in, "rounds": args.rounds, "window_ms": args.window_ms}
        for k, v in times.items():
            v = np.array(v)
            res[k] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                      "p90_ms": round(float(np.percentile(v, 90)), 4), "calls_per_window": inner[k]}
            if k in chunks:
                res[k]["chunk"] = chunks[k]
                res[k]["handed_to_exact"] = handed[k]
        res["decode_kernel"] = ez.decompress_kernel_last()
        res["query_below_decode"] = res["query"]["p90_ms"] < res["decode"]["p10_ms"]
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del data, packed, out


if __name__ == "__main__":
    main()
