"""K2b against the size query: the time of the batch Break index (ez_stream_breaks_batch), of
ez_decompressed_size_batch on the same batch (the same bytes walked once) and of the Break index
without a workspace (the exact decoder alone: what a caller had to pay before).

    python tools/breaks_bench.py [--streams 4096] [--stream-bytes 65536] [--every 512] [--runs 20] [--out FILE]

Two batches of log streams written by the oracle's Writer: one with a Break every ~`every` bytes of
text, and the same text without any Break.  Each call is timed with device events, alternating the
three calls in one loop after a warm-up; the median of the runs is reported with the 10th and 90th
percentiles as the run-to-run spread.  The query's arrays are checked first: with and without a
workspace they are equal, the sizes are the stream lengths, and the Break counts are the ones
written.  One JSON line per batch, with the hash of the kernel sources.

    python tools/breaks_bench.py --shapes b1x16m,b8x2m,... [--route [--forced]] [--rounds 15] [--cache DIR] [--out FILE]

measures the call on a few long framed logs instead (tools/segments_bench.py's method: the legs
alternate in one loop after a warm-up, each timed window repeats its call until it lasts about 20 ms,
median [p10 - p90]).  A shape is `streams` streams of `units` log streams joined back to back (a Writer
that was Reset: each unit starts with its own header), a unit ≈ 0.5 MB compressed (≈ 126 KB in
b4096x126k), written by the oracle's Writer with a Break every ~`every` bytes of text, and the same text
without any Break; 8 distinct units, repeated (--cache keeps them between runs).  Legs:
    call           ez_stream_breaks_batch with every hint (max_len, in_bytes) and no route forced;
    v              (--route) the same under ez_select_breaks_route('v'): a wave per stream;
    p256, p1024    (--route --forced) the parts route forced, at chunk 256 (no max_len) and 1,024;
    size_query, segment_query  (--route) ez_decompressed_size_batch and ez_stream_segments_batch on the
                   same batch with in_bytes (their parts routes where their rules pick them), for scale.
The arrays are checked first: sizes, statuses and Break counts against what was written, every leg's
brk_idx and brk_pos equal to the first leg's.  A library without the route (EZ_LIB pointing at the
parent commit's build) runs the `call` leg alone with in_bytes 0: the baseline, in a process of its
own over the same seeded batches.  One JSON line per shape and variant with the route's counters.
Needs a GPU; there is no fallback."""

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SOURCES = ("ez_decompress_brk.hip", "ez_decompress_brk_parts.hip", "ez_k2_brk_parts.h", "ez_k2_brk_walk.h", "ez_k2_segs_parts.h", "ez_k2_parts.h", "ez_k2_brk.h", "ez_k2_segs.h", "ez_k2_size.h", "ez_k2_walk.h", "ez_k2_parse.h", "ez_decompress.hip",
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


# --shapes: name -> (streams, units per stream, text bytes of a unit); a unit's text compresses about 3.7 : 1
UNIT_TEXT, SMALL_TEXT, DISTINCT = 1_900_000, 466_000, 8
SHAPES = {"b1x16m": (1, 32, UNIT_TEXT), "b8x2m": (8, 4, UNIT_TEXT), "b64x2m": (64, 4, UNIT_TEXT), "b1x05m": (1, 1, UNIT_TEXT),
          "b8x05m": (8, 1, UNIT_TEXT), "b64x05m": (64, 1, UNIT_TEXT), "b256x2m": (256, 4, UNIT_TEXT), "b1024x05m": (1024, 1, UNIT_TEXT),
          "b4096x126k": (4096, 1, SMALL_TEXT)}


def units(text_bytes, every, cache):
    """DISTINCT log streams of text_bytes of text by the oracle's Writer, with a Break every ~`every` bytes
    and without -> {"breaks": [(stream, Breaks)], "no_breaks": [(stream, 0)]}; kept in `cache` where given."""
    import numpy as np

    path = os.path.join(cache, f"units_{text_bytes}_{every}.npz") if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return {v: [(z[f"{v}_{k}"].tobytes(), int(z[f"{v}_n"][k])) for k in range(DISTINCT)] for v in ("breaks", "no_breaks")}
    got = build_batches(DISTINCT, text_bytes, every, DISTINCT)
    res = {v: list(zip(*got[v])) for v in got}
    if path:
        os.makedirs(cache, exist_ok=True)
        keep = {f"{v}_{k}": np.frombuffer(res[v][k][0], np.uint8) for v in res for k in range(DISTINCT)}
        keep.update({f"{v}_n": np.array([n for _, n in res[v]]) for v in res})
        np.savez(path, **keep)
    return res


def run_shapes(args):
    import ctypes as C

    import numpy as np
    import torch

    import eazy_amd as ez

    if not torch.cuda.is_available():
        raise SystemExit("breaks_bench: no GPU")
    dev = torch.device("cuda:0")
    L = ez._lib()
    routed_lib = hasattr(L, "ez_select_breaks_route")  # (else the parent commit's build: the baseline leg alone)
    sp = ez._stream_ptr(None)

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    for name in args.shapes.split(","):
        count, per, text_bytes = SHAPES[name]
        made = units(text_bytes, args.every, args.cache)
        for variant in ("breaks", "no_breaks"):
            us = made[variant]
            arrs = [np.frombuffer(u, np.uint8) for u, _ in us]
            pick = [[(s * per + i) % DISTINCT for i in range(per)] for s in range(count)]
            lens = np.array([sum(len(arrs[k]) for k in p) for p in pick], dtype=np.int64)
            counts = [sum(us[k][1] for k in p) for p in pick]
            coff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            comp = torch.from_numpy(np.concatenate([arrs[k] for p in pick for k in p] + [np.zeros(16, np.uint8)])).to(dev)
            d_coff = torch.from_numpy(coff).to(dev)
            d_ooff = torch.from_numpy(np.arange(count + 1, dtype=np.int64) * (per * text_bytes)).to(dev)
            in_bytes, max_in, found, nseg = int(coff[-1]), int(lens.max()), sum(counts), 4 * count * per + 64  # (room for the segments)
            sizes = torch.empty(count, dtype=torch.int64, device=dev)
            status = torch.empty(count, dtype=torch.int32, device=dev)
            brk_idx = torch.empty(count + 1, dtype=torch.int64, device=dev)
            brk_pos = torch.empty(found + 1, dtype=torch.int64, device=dev)
            brk_total = torch.empty(2, dtype=torch.int64, device=dev)
            seg = [torch.empty(n, dtype=torch.int64, device=dev) for n in (count + 1, nseg + 1, nseg + 1, 2)]
            ws = torch.empty(L.ez_breaks_workspace(count), dtype=torch.uint8, device=dev)
            zws = torch.empty(L.ez_decompress_workspace(count), dtype=torch.uint8, device=dev)
            qws = torch.empty(L.ez_segments_workspace(count), dtype=torch.uint8, device=dev)

            def batch(max_len, hint, out_off=None):
                return ez._Batch(comp.data_ptr(), d_coff.data_ptr(), None, out_off, sizes.data_ptr(), status.data_ptr(), count, max_len, hint, 0)

            def breaks(b, route=None):
                def call():
                    if route is not None:
                        ez.select_breaks_route(route)
                    try:
                        st = L.ez_stream_breaks_batch(0, C.byref(b), brk_idx.data_ptr(), brk_pos.data_ptr(), found + 1, brk_total.data_ptr(),
                                                      ws.data_ptr(), sp)
                        assert st == ez.OK, st
                    finally:
                        if route is not None:
                            ez.select_breaks_route("")
                return call

            zb, gb = batch(max_in, in_bytes), batch(max_in, in_bytes, d_ooff.data_ptr())

            def size_query():
                ez._check(L.ez_decompressed_size_batch(0, C.byref(zb), zws.data_ptr(), sp))

            def segment_query():
                ez._check(L.ez_stream_segments_batch(0, C.byref(gb), seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(), nseg, seg[3].data_ptr(),
                                                     qws.data_ptr(), sp))

            legs = {"call": breaks(batch(max_in, in_bytes if routed_lib else 0))}
            if args.route and routed_lib:
                legs["v"] = breaks(batch(max_in, in_bytes), "v")
                if args.forced:
                    legs["p256"] = breaks(batch(0, in_bytes), "p")
                    legs["p1024"] = breaks(batch(1 << 20, in_bytes), "p")
                legs["size_query"] = size_query
                legs["segment_query"] = segment_query
            first, parts_last = None, {}
            for k, fn in legs.items():  # results first
                sizes.fill_(-1)
                brk_pos.fill_(-1)
                fn()
                torch.cuda.synchronize()
                if k == "segment_query":
                    t = seg[3].cpu().tolist()
                    assert t[0] == t[1] >= count * per, (name, variant, t)
                    continue
                assert sizes.cpu().numpy().tolist() == [per * text_bytes] * count and int(status.abs().sum()) == 0, (name, variant, k)
                if k == "size_query":
                    continue
                got = (brk_idx.cpu().numpy().copy(), brk_pos.cpu().numpy().copy(), tuple(int(v) for v in brk_total.cpu().numpy()))
                assert got[2] == (found, found) and np.diff(got[0]).tolist() == counts, (name, variant, k)
                first = first or got
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (name, variant, k)
                if routed_lib:
                    parts_last[k] = list(ez.breaks_parts_last())
            inner = {}
            for k, fn in legs.items():
                for _ in range(args.warmup):
                    t = timed(fn, 1)
                inner[k] = max(1, min(200, int(args.window_ms / max(t, 1e-3))))
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    times[k].append(timed(fn, inner[k]))
            res = {"shape": name, "batch": variant, "library": "this tree" if routed_lib else "parent", "streams": count, "units_per_stream": per,
                   "unit_text_bytes": text_bytes, "compressed_bytes": in_bytes, "longest_compressed_stream": max_in, "breaks_found": found,
                   "chunk": ez.decompressed_size_chunk(max_in), "rounds": args.rounds, "window_ms": args.window_ms,
                   "device": torch.cuda.get_device_name(0), "kernel_source_sha256_16": source_hash(), "parts_last": parts_last}
            for k, v in times.items():
                v = np.array(v)
                res[k] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                          "p90_ms": round(float(np.percentile(v, 90)), 4), "calls_per_window": inner[k]}
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del comp, brk_pos
            ez.release_cached()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None, help="the long-log shapes instead (see above), comma-separated: " + ",".join(SHAPES))
    ap.add_argument("--route", action="store_true", help="with --shapes: also the wave route, the size query and the segment query")
    ap.add_argument("--forced", action="store_true", help="with --shapes --route: also the parts route forced at chunk 256 and 1,024")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--cache", default=None, help="with --shapes: a directory that keeps the written units")
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--every", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64, help="different streams the host writes; the batch repeats them")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.shapes:
        return run_shapes(args)

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
