#!/usr/bin/env python3
"""Gated live inference timings (docs/PERF.md "Gated live inference").

    python tools/live_gate_bench.py [--model MTL] [--fiber 1000] [--stride 100,125] [--batch 32] [--ring 4096]

Times ``LiveRecording.push`` of 2,000-sample chunks on the engine: ungated (every window evaluated), and -- where the
build has the live gate -- with ``gate_db=3`` under a fixed floor of 1.0 on unit noise in which about 10 %, 50 % and
100 % of the fiber rows are 4x louder (so that share of the windows is active), and with the running floor under a
gate that keeps everything (its three launches and the floor's on top of the ungated work).  The modes alternate,
several rounds each; host clock around ``push``, which ends in the device-to-host copy of its rows, synchronised
before and after, after untimed pushes of the same size.  A build without ``LiveRecording(gate_db=...)`` (the parent
of the change) runs the ungated mode alone: the baseline.  Prints one JSON line.
"""
import argparse
import inspect
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=10, help="timed pushes per mode and round")
    args = ap.parse_args()
    import torch
    from mtl_das_pytorch_amd.inference import LiveRecording
    from mtl_das_pytorch_amd.models import build_model

    torch.manual_seed(0)
    m = build_model(args.model).eval()
    F, B = args.fiber, args.batch
    stride = tuple(int(v) for v in args.stride.split(","))
    n = 2000 - 2000 % stride[1]
    gated = "gate_db" in inspect.signature(LiveRecording.__init__).parameters
    g = torch.Generator().manual_seed(1)
    noise = torch.randn(1, F, n, generator=g)

    def chunk(share):
        x = noise.clone()
        x[:, :int(round(share * F))] *= 4  # loud fiber rows: that share of the (non-overlapping) fiber windows
        return x

    kw = dict(stride=stride, ring=args.ring, batch=B, device="cuda", use_engine=True)
    modes = {"ungated": (chunk(1.0), {})}
    if gated:
        for share in (0.1, 0.5, 1.0):
            modes[f"fixed_floor_{int(100 * share)}"] = (chunk(share), dict(gate_db=3.0, noise_floor=1.0))
        modes["running_floor_keep_all"] = (chunk(1.0), dict(gate_db=-100.0, noise_floor="running"))
    lives = {k: (LiveRecording(m, args.model, F, **kw, **gate), x) for k, (x, gate) in modes.items()}
    times, info = {k: [] for k in lives}, {}
    for live, x in lives.values():  # untimed pushes of the timed size
        for _ in range(4):
            live.push(x)
    for _ in range(args.rounds):
        for k, (live, x) in lives.items():
            for _ in range(args.pushes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = live.push(x)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
            info[k] = {"windows": len(res["positions"]),
                       "active": int(res["active"].sum()) if "active" in res else len(res["positions"])}
    out = {"model": args.model, "fiber": F, "stride": stride, "batch": B, "ring": args.ring, "chunk": n,
           "gated_build": gated}
    for k, ts in times.items():
        out[k] = dict(info[k], median_ms=round(1e3 * statistics.median(ts), 4), min_ms=round(1e3 * min(ts), 4),
                      max_ms=round(1e3 * max(ts), 4), n=len(ts), captures=lives[k][0].captures)
    for live, _ in lives.values():
        live.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
