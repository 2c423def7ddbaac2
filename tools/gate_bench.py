#!/usr/bin/env python3
"""Activity-gated against ungated recording inference (docs/PERF.md "Activity-gated recording inference").

    python tools/gate_bench.py [--model MTL] [--shape 200,20000] [--stride 100,125] [--batch 32] [--loud 0.0875]

Unit noise with a 4x louder stretch of ``--loud`` of the time axis in the middle; ``predict_recording`` on one kept
``window_runner`` with ``gate_db=None`` and with ``gate_db=3, noise_floor=1.0``, in one process: three alternating
groups of one untimed call (a change of mode re-captures the graph) and ``--runs`` timed ones, host clock around the
call, synchronised before and after (upload, power, selection, replays, the table's copy back).  Then
``window_power`` alone: device events around 50 launches.  Prints one JSON line.
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
    ap.add_argument("--shape", default="200,20000")
    ap.add_argument("--stride", default="100,125")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loud", type=float, default=0.0875, help="share of the time axis that is 4x louder")
    args = ap.parse_args()
    import numpy as np
    import torch
    from mtl_das_pytorch_amd.inference import WINDOW, predict_recording, window_runner, window_starts
    from mtl_das_pytorch_amd.models import build_model
    from mtl_das_pytorch_amd.ops import functional as HF
    torch.manual_seed(0)
    model = build_model(args.model).eval()
    shape = tuple(int(v) for v in args.shape.split(","))
    stride = tuple(int(v) for v in args.stride.split(","))
    rec = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    t0 = int(shape[1] * (0.5 - args.loud / 2))
    rec[:, t0:t0 + int(shape[1] * args.loud)] *= 4
    rec = torch.from_numpy(rec)
    dev = torch.device("cuda")
    runner = window_runner(model, args.model, args.batch, dev)

    def call(**gate):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = predict_recording(model, args.model, rec, stride=stride, batch=args.batch, device=dev, use_engine=True,
                                windows="resident", runner=runner, **gate)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t

    modes = {"ungated": {}, "gated": dict(gate_db=3.0, noise_floor=1.0)}
    times = {k: [] for k in modes}
    for _ in range(3):
        for name, kw in modes.items():
            call(**kw)  # untimed
            for _ in range(args.runs):
                res, dt = call(**kw)
                times[name].append(dt)
            if name == "gated":
                share = float(res["active"].mean())
    n = len(res["positions"])
    out = {"model": args.model, "shape": shape, "stride": stride, "batch": args.batch, "windows": n,
           "active_share": round(share, 4)}
    for name, t in times.items():
        out[name] = {"median_ms": round(1e3 * statistics.median(t), 3), "min_ms": round(1e3 * min(t), 3),
                     "max_ms": round(1e3 * max(t), 3), "n": len(t)}
    fs, ts = window_starts(shape[0], WINDOW[0], stride[0]), window_starts(shape[1], WINDOW[1], stride[1])
    rec_d = rec.unsqueeze(0).to(dev)
    for _ in range(3):
        HF.window_power(rec_d, fs, ts, WINDOW)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        HF.window_power(rec_d, fs, ts, WINDOW)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 50
    # both passes read every element of every window
    out["window_power"] = {"ms": round(ms, 4), "read_GB_per_s": round(2 * n * WINDOW[0] * WINDOW[1] * 4 / ms / 1e6, 1)}
    runner.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
