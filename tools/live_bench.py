#!/usr/bin/env python3
"""Live inference timings (docs/PERF.md "Live inference").

    python tools/live_bench.py [--model MTL] [--fiber 1000] [--stride 100,125] [--batch 32] [--ring 4096]

Times ``LiveRecording.push`` on the engine for a chunk of one time stride (one time index: a partial batch when the
fiber has fewer windows than the batch) and for a chunk of 2,000 samples, from the host and from the device, without
and with the map; then ``predict_recording`` on a kept ``window_runner`` and a ``LiveRecording`` stream on the same
recording.  Host clock around calls that end in the device-to-host copy of their results, synchronised before and
after, each size after untimed calls of the same size.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="MTL")
    ap.add_argument("--fiber", type=int, default=1000)
    ap.add_argument("--stride", default="100,125")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ring", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from mtl_das_pytorch_amd.inference import WINDOW, LiveRecording, predict_recording, window_runner
    from mtl_das_pytorch_amd.models import build_model

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    def stats(ts):
        return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
                "max_ms": round(1e3 * max(ts), 4), "n": len(ts)}

    torch.manual_seed(0)
    m = build_model(args.model).eval()
    F, B = args.fiber, args.batch
    stride = tuple(int(v) for v in args.stride.split(","))
    big_n = 2000 - 2000 % stride[1]
    out = {"model": args.model, "fiber": F, "stride": stride, "batch": B, "ring": args.ring}
    g = torch.Generator().manual_seed(1)
    small, big = torch.randn(1, F, stride[1], generator=g), torch.randn(1, F, big_n, generator=g)
    live_kw = dict(stride=stride, ring=args.ring, batch=B, device="cuda", use_engine=True)
    for cell in (None, stride):
        for where in ("host", "device"):
            live = LiveRecording(m, args.model, F, cell=cell, **live_kw)
            a, b = (small, big) if where == "host" else (small.cuda(), big.cuda())
            live.push(b)
            for _ in range(5):
                live.push(a)
            nwin = []
            ts = timed(lambda: nwin.append(len(live.push(a)["positions"])), 40)
            tag = f"{'map' if cell else 'nomap'}_{where}"
            out[f"push{stride[1]}_{tag}"] = dict(stats(ts), windows=nwin[-1])
            for _ in range(3):
                live.push(b)
            nwin = []
            ts = timed(lambda: nwin.append(len(live.push(b)["positions"])), 20)
            out[f"push{big_n}_{tag}"] = dict(stats(ts), windows=nwin[-1])
            out["captures"] = live.captures
            live.close()
    # the whole recording on a kept runner, and the same recording as a stream of big chunks
    T = WINDOW[1] + stride[1] * 160
    rec = torch.randn(F, T, generator=g)
    runner = window_runner(m, args.model, B, torch.device("cuda"))

    def offline():
        return predict_recording(m, args.model, rec, stride=stride, batch=B, device="cuda", use_engine=True,
                                 runner=runner)
    n = len(offline()["positions"])
    offline()
    ts = timed(offline, 8)
    out["offline"] = dict(stats(ts), windows=n, windows_per_s=round(n / statistics.median(ts), 1))
    runner.close()
    live = LiveRecording(m, args.model, F, **live_kw)

    def stream():
        return sum(len(live.push(rec[:, t:t + big_n])["positions"]) for t in range(0, T, big_n))
    stream()
    cnts = []
    ts = timed(lambda: cnts.append(stream()), 5)
    out["live_stream"] = dict(stats(ts), windows=cnts[-1], windows_per_s=round(cnts[-1] / statistics.median(ts), 1))
    live.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
