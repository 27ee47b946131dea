"""The first Read of a NewReaderBytes handle: its latency and the device memory the handle holds
afterwards, on the streams where the whole-stream slot matters:

    log16    a 16 MiB log stream                        (eazy_amd/synth.py, about 2 : 1)
    dense16  16 MiB that compress about 20 : 1          (runs of zeros between log lines)
    rand16   16 MiB of incompressible bytes
    bomb     a stream of under 200 bytes that decodes to over 10 GiB

    python tools/reader_first_read.py [--rounds 9] [--out FILE]

Per stream and round a fresh handle reads 64 KiB once; the time is the host clock around that Read
(ez_reader_read returns after a synchronise).  The device memory is the drop in free memory
(hipMemGetInfo through torch) from before the handle exists to after the Read, with the library's
caches released before each measurement.  One JSON line per stream: median [p10 - p90] in ms, the
device bytes, and what the handle says of its whole-stream attempt where the library reports it.
Needs a GPU; there is no fallback."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--label", default="", help="a name for the build under measurement")
    args = ap.parse_args()

    import numpy as np
    import torch

    import eazy_amd as ez
    import oracle as orc
    from eazy_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("reader_first_read: no GPU")
    torch.cuda.init()
    L = ez._lib()
    have = hasattr(L, "ez_reader_whole_slot")

    def stream(plain):
        dev = torch.device("cuda:0")
        data = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).to(dev)
        off = torch.tensor([0, len(plain)], dtype=torch.int64, device=dev)
        cb = ez.compress_batch(data, off, ez.MiB, 1024, max_len=len(plain))
        packed, poff = ez.pack(cb)
        torch.cuda.synchronize()
        assert int(cb.status.abs().sum()) == 0
        return packed.cpu().numpy()[: int(poff[1].item())].tobytes()

    n = 16 << 20
    logs = synth.logs(5, n).tobytes()
    dense = bytearray()
    k = 0
    while len(dense) < n:
        dense += logs[k : k + 800] + bytes(16000)
        k += 800
    rng = np.random.default_rng(7)
    hdr = b"\x80\x02eazy\x80\x10\x14"
    E = ez.Encoder()
    bomb = hdr + E.tag(b"", 0, 1) + b"x" + E.offset(E.tag(b"", 0x80, 1 << 29), 1, 1 << 29) * 20
    cases = [("log16", stream(logs), n), ("dense16", stream(bytes(dense[:n])), n),
             ("rand16", stream(rng.integers(0, 256, n, dtype=np.uint8).tobytes()), n), ("bomb", bomb, None)]
    for name, b, want in cases:
        times, held, info = [], [], {}
        for _ in range(args.rounds + 1):  # (the first round warms the library up and is dropped)
            ez.release_cached() if hasattr(ez, "release_cached") else L.ez_release_cached(-1)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            r = ez.Reader(b=b)
            t0 = time.perf_counter()
            got, err = r.Read(65536)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            held.append(free0 - torch.cuda.mem_get_info()[0])
            times.append(1e3 * (t1 - t0))
            assert len(got) == 65536 and err == ez.OK, (name, len(got), err)
            info = {"whole_decoded": bool(r.whole_decoded)}
            if have:
                info.update(whole_slot=r.whole_slot, whole_launches=r.whole_launches)
            del r
        v = np.array(times[1:])
        res = {"build": args.label, "stream": name, "compressed_bytes": len(b), "decoded_bytes": want, "rounds": args.rounds,
               "first_read_median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
               "p90_ms": round(float(np.percentile(v, 90)), 3), "device_bytes_held": int(np.median(held[1:])), **info}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
