#!/usr/bin/env python3
"""Resident-recording inference against the materialised window stack (docs/PERF.md "Resident-recording inference").

    python tools/infer_bench.py [--model MTL] [--shape 400,10000] [--stride 20,50] [--batch 32] [--runs 5]

Times ``predict_recording(..., use_engine=True)`` with ``windows="resident"`` and ``windows="materialize"`` in one
process, each after one untimed call: the median of ``--runs`` calls, synchronised before and after, and the
growth of the allocator's peak across a call.  Every call lowers the model and captures its graph, as the CLI does
once per recording; ``resident, one runner`` is the same work on a ``window_runner`` kept over the calls.  Prints
one JSON line.
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
    ap.add_argument("--shape", default="400,10000")
    ap.add_argument("--stride", default="20,50")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    from mtl_das_pytorch_amd.inference import predict_recording, window_runner
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(args.model).eval()
    shape = tuple(int(v) for v in args.shape.split(","))
    stride = tuple(int(v) for v in args.stride.split(","))
    rec = torch.randn(*shape)
    dev = torch.device("cuda")
    runner = window_runner(model, args.model, args.batch, dev)
    settings = {"materialize": dict(windows="materialize"), "resident": dict(windows="resident"),
                "resident, one runner": dict(windows="resident", runner=runner)}
    out = {"model": args.model, "shape": shape, "stride": stride, "batch": args.batch, "runs": args.runs}
    for name, kw in settings.items():
        def call():
            return predict_recording(model, args.model, rec, stride=stride, batch=args.batch, device=dev,
                                     use_engine=True, **kw)
        n = len(call()["positions"])  # untimed
        times, grow = [], []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            grow.append(torch.cuda.max_memory_allocated() - base)
        med = statistics.median(times)
        out["windows"] = n
        out[name] = {"windows_per_s": round(n / med, 1), "median_s": round(med, 4),
                     "min_s": round(min(times), 4), "max_s": round(max(times), 4),
                     "peak_growth_MB": round(max(grow) / 1e6, 2)}
    runner.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
