#!/usr/bin/env python3
"""Live inference timings (docs/PERF.md "Live inference").

    python tools/live_bench.py [--model MTL] [--fiber 1000] [--stride 100,125] [--batch 32] [--ring 4096]

Times ``LiveRecording.push`` on the engine for a chunk of one time stride (one time index: a partial batch when the
fiber has fewer windows than the batch) and for a chunk of 2,000 samples, from the host and from the device, without
and with the map; then ``predict_recording`` on a kept ``window_runner`` and a ``LiveRecording`` stream on the same
recording.  Host clock around calls that end in the device-to-host copy of their results, synchronised before and
after, each size after untimed calls of the same size.  Prints one JSON line.

    python tools/live_bench.py --decimate 10

adds ``decimate``: the ``fir_decimate`` launch alone on 2,000 * D raw samples per row (fp32 and int16 input; the
default taps and ``taps = [1]``) beside a device-to-device copy of the same raw bytes timed in the same run -- every
raw sample has to be read once, so the copy is the floor -- and ``LiveRecording.push`` of that raw chunk from the host
beside a push of the 2,000 decimated samples without decimation.

    python tools/live_bench.py --common_mode median

adds ``common_mode``: the ``common_mode`` launch alone, in place as the live path runs it, on the chunk shape above
(``--fiber`` rows of 2,000 columns) and on four times the rows -- the work is linear in the fiber, so the ratio should
be about 4 -- beside a device-to-device copy of the same bytes (the floor: every sample is read and written once);
these are device-event times over 20 launches back to back, so the launch overhead of a single call is not in
them.  Then ``LiveRecording.push`` of the chunk from the host with the stage and without it, alternating.
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
    ap.add_argument("--decimate", type=int, default=None, help="also time the raw-rate front end at this factor")
    ap.add_argument("--common_mode", choices=["median", "mean"], default=None,
                    help="also time the common-mode stage with this estimate")
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
    if args.decimate is not None:
        out["decimate"] = decimate_timings(args, m, stride, timed, stats)
    if args.common_mode is not None:
        out["common_mode"] = common_mode_timings(args, m, stride, timed, stats)
    print(json.dumps(out))


def decimate_timings(args, model, stride, timed, stats):
    """The raw-rate front end at factor ``--decimate``: launch, copy floor and push (module docstring)."""
    import torch
    from mtl_das_pytorch_amd.data.resample import as_taps
    from mtl_das_pytorch_amd.inference import LiveRecording
    from mtl_das_pytorch_amd.ops import functional as HF
    D, F, n_out = args.decimate, args.fiber, 2000
    g = torch.Generator().manual_seed(2)
    res = {"D": D, "fiber": F, "raw_per_row": n_out * D}
    raws = {"fp32": torch.randn(1, F, n_out * D, generator=g),
            "int16": torch.randint(-3000, 3000, (1, F, n_out * D), generator=g).to(torch.int16)}
    for name, taps in (("default", as_taps(None, D)), ("one", as_taps([1.0], D))):
        taps_d = torch.from_numpy(taps).cuda()
        for kind, raw in raws.items():
            raw_d = raw.cuda()
            m = (raw_d.shape[2] - len(taps)) // D + 1
            dst = torch.empty(1, F, m, device="cuda")
            carry = HF.decimate_carry(F, len(taps), "cuda")
            for _ in range(5):
                HF.fir_decimate(raw_d, carry[0], 0, 0, taps_d, D, out=dst, m=m, carry_out=carry[1])
            ts = timed(lambda: HF.fir_decimate(raw_d, carry[0], 0, 0, taps_d, D, out=dst, m=m, carry_out=carry[1]), 50)
            res[f"launch_{name}_{kind}"] = dict(stats(ts), taps=len(taps), outputs=m)
    for kind, raw in raws.items():
        raw_d, twin = raw.cuda(), torch.empty_like(raw, device="cuda")
        for _ in range(5):
            twin.copy_(raw_d)
        res[f"copy_{kind}"] = dict(stats(timed(lambda: twin.copy_(raw_d), 50)), bytes=raw.numel() * raw.element_size())
    # push from the host: the raw chunk with the front end, and its 2,000 decimated samples without
    big_n = n_out - n_out % stride[1]
    live_kw = dict(stride=stride, ring=args.ring, batch=args.batch, device="cuda", use_engine=True)
    plain = torch.randn(1, F, big_n, generator=g)
    runs = [("push_plain", {}, plain)]
    runs += [(f"push_raw_{kind}", {"decimate": D}, raw[:, :, :big_n * D].contiguous()) for kind, raw in raws.items()]
    for tag, kw, chunk in runs:
        live = LiveRecording(model, args.model, F, **live_kw, **kw)
        for _ in range(4):
            live.push(chunk)
        nwin = []
        ts = timed(lambda: nwin.append(len(live.push(chunk)["positions"])), 20)
        res[tag] = dict(stats(ts), windows=nwin[-1], samples=chunk.shape[2])
        live.close()
    return res


def common_mode_timings(args, model, stride, timed, stats):
    """The common-mode stage with ``--common_mode``: launch and copy floor at F and 4 F rows, and the push with and
    without it (module docstring)."""
    import torch
    from mtl_das_pytorch_amd.inference import LiveRecording
    from mtl_das_pytorch_amd.ops import functional as HF
    how, F, n, reps = args.common_mode, args.fiber, 2000, 20
    g = torch.Generator().manual_seed(3)
    res = {"how": how, "columns": n, "launches_per_timing": reps}

    def events(fn, rounds=10):
        """Device time of one ``fn()``, ms: ``reps`` calls back to back between two events, ``rounds`` times."""
        for _ in range(3):
            fn()
        ts = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / reps / 1e3)
        return stats(ts)
    for rows in (F, 4 * F):
        x = torch.randn(1, rows, n, generator=g).cuda()
        twin, trace = torch.empty_like(x), torch.empty(1, n, device="cuda")
        # in place: after the first launch the data is its own residue, still noise of the same spread
        res[f"launch_F{rows}"] = dict(events(lambda: HF.common_mode(x, how, out=x, trace=trace)), bytes=4 * x.numel())
        res[f"copy_F{rows}"] = dict(events(lambda: twin.copy_(x)), bytes=4 * x.numel())
    res["launch_ratio_4F"] = round(res[f"launch_F{4 * F}"]["median_ms"] / res[f"launch_F{F}"]["median_ms"], 3)
    # push from the host, the stage on and off in alternating groups
    big_n = n - n % stride[1]
    chunk = torch.randn(1, F, big_n, generator=g)
    live_kw = dict(stride=stride, ring=args.ring, batch=args.batch, device="cuda", use_engine=True)
    lives = {"push_plain": LiveRecording(model, args.model, F, **live_kw),
             "push_common_mode": LiveRecording(model, args.model, F, common_mode=how, **live_kw)}
    ts = {k: [] for k in lives}
    for live in lives.values():
        for _ in range(4):
            live.push(chunk)
    for _ in range(4):
        for k, live in lives.items():
            ts[k] += timed(lambda: live.push(chunk), 5)
    for k, live in lives.items():
        res[k] = dict(stats(ts[k]), samples=big_n, captures=live.captures)
        live.close()
    return res


if __name__ == "__main__":
    main()
