"""K2z's parts route against its wave route (tools/size_bench.py's method: alternating rounds in one
process, device events, median [p10 - p90]) on the shapes where few long streams leave the wave route
most of the chip idle, and on two where they do not:

    c4s     64 x 4 MiB fp32 buckets, 90 % zeros          (bench.py's generator)
    c4      64 x 4 MiB fp32 buckets                      (bench.py's generator)
    log05, log1, log4, log16, log64   one log stream of 0.5, 1, 4, 16, 64 MiB   (eazy_amd/synth.py)
    log1k   1,024 x 1 MiB log streams
    c2      4,096 x 256 KiB log streams                  (bench.py's generator)

    python tools/size_parts_bench.py [--shapes c4s,c4,log05,log1,log4,log16,log64,log1k,c2] [--rounds 15] [--out FILE]

Per shape the batch is compressed on the device (compress_batch + pack) and then, alternating in one
loop after a warm-up: the query on the wave route under the hint a caller would give (route 'v': the
code every query ran before the parts route existed), the query on the parts route with chunk 256
and with chunk 1,024 (route 'p', in_bytes given), the query as the library routes it (automatic,
in_bytes given), and the decode.  Each timed window repeats its call until it lasts about 20 ms.
Every leg's sizes are checked against the stream lengths.  One JSON line per shape: medians in ms,
the 10th and 90th percentiles as the run-to-run spread, the parts route's counters (parts walked,
taken as recorded, walked again) and, per chunk, whether the parts route's p90 lies below the wave
route's p10.  Needs a GPU; there is no fallback."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOGS = {"log05": (1, 512 << 10), "log1": (1, 1 << 20), "log4": (1, 4 << 20), "log16": (1, 16 << 20), "log64": (1, 64 << 20), "log1k": (1024, 1 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4s,c4,log05,log1,log4,log16,log64,log1k,c2")
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
        raise SystemExit("size_parts_bench: no GPU")
    dev = torch.device("cuda:0")

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    for name in args.shapes.split(","):
        if name in LOGS:
            count, size = LOGS[name]
            block, htable, desc = 1 << 20, 1024, f"{name}: {count} x {size >> 10} KiB log-like streams, block 1 MiB, htable 1024"
            host = synth.logs(1, count * size)
        else:
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
        comp_len = poff[1:] - poff[:-1]
        max_in, in_bytes = int(comp_len.max().item()), int((poff[-1] - poff[0]).item())
        out = torch.empty(count * size + 16, dtype=torch.uint8, device=dev)
        dsz = torch.empty(count, dtype=torch.int64, device=dev)
        dst = torch.empty(count, dtype=torch.int32, device=dev)
        qsz = torch.empty(count, dtype=torch.int64, device=dev)
        qst = torch.empty(count, dtype=torch.int32, device=dev)
        ws = torch.empty(ez._lib().ez_decompress_workspace(count), dtype=torch.uint8, device=dev)

        def query(route, hint, nin):
            def run():
                ez.select_size_route(route)
                ez.decompressed_sizes(packed, poff, sizes=qsz, status=qst, workspace=ws, max_len=hint, in_bytes=nin)
                ez.select_size_route("")

            return run

        def decode():
            ez.decompress_batch(packed, poff, off, out=out, sizes=dsz, status=dst, workspace=ws, max_len=size, in_bytes=in_bytes,
                                out_bytes=count * size)

        # (a forced parts route takes chunk 1,024 where the wave route does, above 512 KiB, else 256)
        legs = {"wave": query("v", max_in, 0), "parts256": query("p", 4097, in_bytes), "parts1024": query("p", 1 << 20, in_bytes),
                "auto": query("", max_in, in_bytes), "decode": decode}
        chunks, parts = {}, {}
        for k, fn in legs.items():  # results first: every leg reports the stream lengths
            qsz.fill_(-1)
            fn()
            torch.cuda.synchronize()
            if k != "decode":
                chunks[k] = ez.decompressed_size_chunk_last()
                parts[k] = list(ez.decompressed_size_parts_last())
                assert int(ws[:4].cpu().numpy().view(np.uint32)[0]) == 0, (name, k)
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
        res = {"shape": name, "desc": desc, "streams": count, "stream_bytes": size, "compressed_bytes": in_bytes,
               "longest_compressed_stream": max_in, "rounds": args.rounds, "window_ms": args.window_ms}
        for k, v in times.items():
            v = np.array(v)
            res[k] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                      "p90_ms": round(float(np.percentile(v, 90)), 4), "calls_per_window": inner[k]}
            if k in chunks:
                res[k]["chunk"] = chunks[k]
                res[k]["parts"] = parts[k]
        res["decode_kernel"] = ez.decompress_kernel_last()
        for k in ("parts256", "parts1024", "auto"):
            res[k + "_below_wave"] = res[k]["p90_ms"] < res["wave"]["p10_ms"]
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del data, packed, out


if __name__ == "__main__":
    main()
