"""The segmented decode (K2g, ez_decompress_batch_segmented) against what a batch of concatenated streams
costs without it (tools/size_parts_bench.py's method: alternating rounds in one process, device events,
median [p10 - p90]).  Log data (eazy_amd/synth.py) in frames of 64 KiB, compressed on the device
(compress_batch + pack) and read with in-offsets that join consecutive frames into one stream:

    s4096x4    4,096 streams of 4 segments
    s1024x16   1,024 streams of 16 segments
    s64x64     64 streams of 64 segments
    s8x64      8 streams of 64 segments
    s1x512     a lone stream of 512 segments
    s256x64, s64x16, s8x16, s1x16   either side of the automatic rule's thresholds (--route)

    python tools/segments_bench.py [--shapes s4096x4,s1024x16,s64x64] [--rounds 15] [--out FILE] [--sized] [--route [--forced]]

Per shape, alternating in one loop after a warm-up:
    batch      decompress_batch with a workspace and every hint: each stream holds a Reset after output,
               so every one lands on the exact decoder (what the call cost before the segment query);
    query      ez_stream_segments_batch alone, with room for every segment;
    segmented  decompress_batch_segmented;
    floor      decompress_batch over the frames as separate streams, the offsets known and every hint given.
Each timed window repeats its call until it lasts about 20 ms.  Every decoding leg's sizes, statuses
and bytes are checked against the data, the query's arrays against the frames' offsets, and the
segmented call's counters (segments, none handed over).  One JSON line per shape: medians in ms, the
10th and 90th percentiles as the run-to-run spread, the query's share of the segmented call, the
segmented call over the floor, and whether the segmented call's p90 lies below the batch call's p10.
--sized measures the caller who knows no decoded lengths instead, two legs on the joined streams:
    sizes         decompressed_sizes with a workspace and the longest stream as its hint;
    sized_decode  decompress_batch_sized (the query, one read-back, the decode).
Their sizes, statuses and bytes are checked, and where the library has the size query's K2g stage
its counters (every stream taken and sized, none handed on) and the segmented decode behind it.  The
mode runs on a build without that stage too, for the comparison.
--route measures the query's routes instead (ez_select_segments_route), alternating in the same loop:
    query_v, segmented_v        the wave route: a wave per stream;
    query_auto, segmented_auto  the automatic rule, with the in_bytes hint that lets the parts route run;
    floor                       as above.
--forced adds query_p256 and query_p1024, the parts route forced at either chunk size (the figures the
automatic rule's thresholds come from).  With --sized the legs are sizes_v / sizes_auto (decompressed_sizes
with in_bytes) and sized_decode_v / sized_decode_auto.  Per automatic leg the line says whether its p90
lies below the wave leg's p10, whether the two [p10 - p90] overlap, and the parts route's counters
(all zero: the rule picked the wave route).
Needs a GPU; there is no fallback."""

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"s4096x4": (4096, 4), "s1024x16": (1024, 16), "s64x64": (64, 64), "s8x64": (8, 64), "s1x512": (1, 512),
          "s256x64": (256, 64), "s64x16": (64, 16), "s8x16": (8, 16), "s1x16": (1, 16)}
FRAME = 64 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s4096x4,s1024x16,s64x64")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--sized", action="store_true", help="measure decompressed_sizes and decompress_batch_sized instead")
    ap.add_argument("--route", action="store_true", help="measure the query's wave route against the automatic rule instead")
    ap.add_argument("--forced", action="store_true", help="with --route: also the parts route forced at chunk 256 and 1,024")
    args = ap.parse_args()

    import numpy as np
    import torch

    import eazy_amd as ez
    from eazy_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("segments_bench: no GPU")
    dev = torch.device("cuda:0")
    L = ez._lib()

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    shapes = [(n,) + SHAPES[n] for n in args.shapes.split(",")]
    most = max(c * g for _, c, g in shapes)
    host = synth.logs(1, most * FRAME)  # one set of frames: a shape takes the first count x segments of them
    for name, count, segs in shapes:
        frames = count * segs
        block, htable = 1 << 20, 1024
        desc = f"{name}: {count} streams of {segs} frames of {FRAME >> 10} KiB of log-like data, block 1 MiB, htable 1024"
        data = torch.from_numpy(np.ascontiguousarray(host[: frames * FRAME])).to(dev)
        off = torch.from_numpy(synth.batch_offsets(frames, FRAME)).to(dev)
        cb = ez.compress_batch(data, off, block, htable, max_len=FRAME)
        packed, poff = ez.pack(cb)
        torch.cuda.synchronize()
        assert int(cb.status.abs().sum()) == 0
        del cb
        joff, jooff = poff[::segs].contiguous(), off[::segs].contiguous()  # the joined streams
        in_bytes = int((poff[-1] - poff[0]).item())
        max_in = int((joff[1:] - joff[:-1]).max().item())
        out = torch.empty(frames * FRAME + 16, dtype=torch.uint8, device=dev)
        sz = {k: torch.empty(n, dtype=torch.int64, device=dev) for k, n in (("j", count), ("f", frames))}
        st = {k: torch.empty(n, dtype=torch.int32, device=dev) for k, n in (("j", count), ("f", frames))}
        ws = torch.empty(L.ez_decompress_workspace(frames), dtype=torch.uint8, device=dev)
        seg_idx = torch.empty(count + 1, dtype=torch.int64, device=dev)
        seg_in = torch.empty(frames + 1, dtype=torch.int64, device=dev)
        seg_out = torch.empty(frames + 1, dtype=torch.int64, device=dev)
        seg_total = torch.empty(2, dtype=torch.int64, device=dev)
        qws = torch.empty(L.ez_segments_workspace(count), dtype=torch.uint8, device=dev)
        qb = ez._Batch(packed.data_ptr(), joff.data_ptr(), None, jooff.data_ptr(), None, None, count, max_in, in_bytes if args.route else 0, 0)
        # (the forced legs: the max_len hint picks the parts route's chunk, 256 without one, 1,024 for a long stream)
        qb256 = ez._Batch(packed.data_ptr(), joff.data_ptr(), None, jooff.data_ptr(), None, None, count, 0, in_bytes, 0)
        qb1024 = ez._Batch(packed.data_ptr(), joff.data_ptr(), None, jooff.data_ptr(), None, None, count, 1 << 20, in_bytes, 0)

        def batch():
            ez.decompress_batch(packed, joff, jooff, out=out, sizes=sz["j"], status=st["j"], workspace=ws, max_len=segs * FRAME,
                                in_bytes=in_bytes, out_bytes=frames * FRAME)

        def query(qb=qb):
            ez._check(L.ez_stream_segments_batch(0, C.byref(qb), seg_idx.data_ptr(), seg_in.data_ptr(), seg_out.data_ptr(), frames,
                                                 seg_total.data_ptr(), qws.data_ptr(), ez._stream_ptr(None)))

        def segmented():
            ez.decompress_batch_segmented(packed, joff, jooff, out=out, sizes=sz["j"], status=st["j"])

        def floor():
            ez.decompress_batch(packed, poff, off, out=out, sizes=sz["f"], status=st["f"], workspace=ws, max_len=FRAME, in_bytes=in_bytes,
                                out_bytes=frames * FRAME)

        def sizes():
            ez.decompressed_sizes(packed, joff, sizes=sz["j"], status=st["j"], workspace=ws, max_len=max_in, in_bytes=in_bytes if args.route else 0)

        def routed(fn, route):
            def leg():
                ez.select_segments_route(route)
                try:
                    return fn()
                finally:
                    ez.select_segments_route("")
            return leg

        def sized_decode():
            return ez.decompress_batch_sized(packed, joff)

        legs = {"batch": batch, "query": query, "segmented": segmented, "floor": floor}
        kernels, last = {}, None
        if args.sized:
            legs = {"sizes": sizes, "sized_decode": sized_decode}
            stage = getattr(ez, "decompressed_size_segs_last", None)  # (None: a build without the stage)
            sizes()
            torch.cuda.synchronize()
            assert sz["j"].cpu().tolist() == [segs * FRAME] * count and int(st["j"].abs().sum()) == 0, name
            counters = list(stage(ws, count)) if stage else None
            assert counters in (None, [count, count, 0]), (name, counters)
            o, oo, osz, ost = sized_decode()
            torch.cuda.synchronize()
            assert osz.cpu().tolist() == [segs * FRAME] * count and int(ost.abs().sum()) == 0, name
            assert torch.equal(oo, jooff) and torch.equal(o[: frames * FRAME], data), name
            last = ez.segments_last() if stage else (0, 0, 0)
            assert not stage or last[:2] == (frames, 0), (name, last)
            kernels = {"sized_decode": ez.decompress_kernel_last(), "stage_counters": counters}
            del o
        if args.route:
            if args.sized:
                legs = {"sizes_v": routed(sizes, "v"), "sizes_auto": sizes, "sized_decode_v": routed(sized_decode, "v"), "sized_decode_auto": sized_decode}
            else:
                legs = {"query_v": routed(query, "v"), "query_auto": query, "segmented_v": routed(segmented, "v"), "segmented_auto": segmented,
                        "floor": floor}
                if args.forced:
                    legs["query_p256"] = routed(lambda: query(qb256), "p")
                    legs["query_p1024"] = routed(lambda: query(qb1024), "p")
        parts_last = {}
        for k, fn in ({} if args.sized else legs).items():  # results first
            out.zero_()
            fn()
            torch.cuda.synchronize()
            if k.startswith("query"):
                parts_last[k] = list(ez.segments_parts_last()) if args.route else None
                assert seg_total.cpu().tolist() == [frames, frames], (name, seg_total.cpu().tolist())
                # (a cut is at the Reset's tag byte: the frame's Magic meta before it stays with the segment before)
                lead = seg_in - poff
                assert int(lead.min()) >= 0 and int(lead.max()) <= 6 and torch.equal(seg_in[::segs], joff) and torch.equal(seg_out, off), name
                assert seg_idx.cpu().tolist() == list(range(0, frames + 1, segs)), name
                continue
            kernels[k] = ez.decompress_kernel_last()
            key = "f" if k == "floor" else "j"
            assert sz[key].cpu().tolist() == [(FRAME if k == "floor" else segs * FRAME)] * (frames if k == "floor" else count), (name, k)
            assert int(st[key].abs().sum()) == 0 and torch.equal(out[: frames * FRAME], data), (name, k)
            if k == "batch":
                assert int(ws[:4].cpu().numpy().view(np.uint32)[0]) == count, (name, "not every stream went to the exact decoder")
            if k.startswith("segmented"):
                last = ez.segments_last()
                assert last[:2] == (frames, 0), (name, last)
        inner = {}
        for k, fn in legs.items():
            for _ in range(args.warmup):
                t = timed(fn, 1)
            inner[k] = max(1, min(200, int(args.window_ms / max(t, 1e-3))))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, inner[k]))
        res = {"shape": name, "desc": desc, "streams": count, "segments": segs, "frame_bytes": FRAME, "compressed_bytes": in_bytes,
               "longest_compressed_stream": max_in, "rounds": args.rounds, "window_ms": args.window_ms, "segments_last_first_call": list(last),
               "segments_last": list(ez.segments_last()), "decode_kernels": kernels}
        for k, v in times.items():
            v = np.array(v)
            res[k] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                      "p90_ms": round(float(np.percentile(v, 90)), 4), "calls_per_window": inner[k]}
        if args.route:
            res["parts_last"] = parts_last
            for k in [k for k in legs if k.endswith("_auto")]:
                a, v = res[k], res[k[:-5] + "_v"]
                res[k + "_below_v"] = a["p90_ms"] < v["p10_ms"]
                res[k + "_overlaps_v"] = a["p10_ms"] <= v["p90_ms"] and v["p10_ms"] <= a["p90_ms"]
        elif not args.sized:
            res["query_share_of_segmented"] = round(res["query"]["median_ms"] / res["segmented"]["median_ms"], 4)
            res["segmented_over_floor"] = round(res["segmented"]["median_ms"] / res["floor"]["median_ms"], 4)
            res["batch_over_segmented"] = round(res["batch"]["median_ms"] / res["segmented"]["median_ms"], 4)
            res["segmented_below_batch"] = res["segmented"]["p90_ms"] < res["batch"]["p10_ms"]
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del data, packed, out
        ez.release_cached()


if __name__ == "__main__":
    main()
