#!/usr/bin/env python3
"""Sliding-window inference over a long DAS recording (fiber x time matrix, .npy or .mat).

    python infer.py --model MTL --model_path run/<...>.pth --recording fiber.npy --stride 100,125 \
        --out predictions.csv --cell 50,125 --map maps.npz
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 infer.py ...   # windows sharded over ranks
    python infer.py ... --chunk 2000 [--ring 4096]   # read and evaluate the recording 2000 time samples at a time
    python infer.py ... --gate_db 3 [--noise_floor auto|P]   # evaluate only windows 3 dB above the noise floor
    python infer.py ... --chunk 2000 --gate_db 3 --noise_floor running [--floor_history 64]   # the gate on the chunked
        # run: the floor is the running median of the last 64 time indices (or --noise_floor P, a fixed power)
    python infer.py ... --decimate 10 [--taps taps.npy] [--chunk 20000]   # the recording is at the raw rate (fp32 or
        # int16): low-pass FIR and decimation by 10 first; --chunk then counts raw samples
    python infer.py ... --common_mode median [--chunk 2000]   # subtract the per-sample median (or mean) over the fiber
        # from the stream the windows are cut from (after --decimate): laser and interrogator noise common to all
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description="Sliding-window DAS inference")
    ap.add_argument("--model", default="MTL", help="MTL, single_event, single_distance, multi_classifier")
    ap.add_argument("--model_path", default=None, help="reference-format state_dict (.pth)")
    ap.add_argument("--recording", required=True, help=".npy ([F, T] or [C, F, T]) or .mat (key --key)")
    ap.add_argument("--key", default="data")
    ap.add_argument("--stride", default="100,125", help="window stride (fiber, time)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--in_channels", type=int, default=1)
    ap.add_argument("--backend", choices=["auto", "engine", "torch"], default="auto")
    ap.add_argument("--out", default="predictions.csv")
    ap.add_argument("--cell", default=None, help="map cell (fiber, time) in samples; default: the stride")
    ap.add_argument("--map", default=None, help="write the event / distance maps of the recording to this .npz")
    ap.add_argument("--chunk", type=int, default=None,
                    help="feed the recording to a LiveRecording in chunks of this many time samples (a .npy is "
                         "memory-mapped): the recording need not fit on the device; same CSV and maps")
    ap.add_argument("--ring", type=int, default=None, help="with --chunk: time samples kept on the device")
    ap.add_argument("--gate_db", type=float, default=None,
                    help="activity gate: only windows whose power is at least the noise floor + this many dB are "
                         "evaluated, the others are reported as quiet (pred -1); default: no gate")
    ap.add_argument("--noise_floor", default="auto",
                    help="with --gate_db: 'auto' (per fiber position, the lower median of its windows' powers over "
                         "time; not with --chunk), 'running' (with --chunk: the lower median of the last "
                         "--floor_history time indices, the window's own included) or a power")
    ap.add_argument("--floor_history", type=int, default=64,
                    help="with --noise_floor running: time indices the running median looks back over")
    ap.add_argument("--floor_warmup", type=int, default=None,
                    help="with --noise_floor running: every window is active until this many time indices exist "
                         "(default: 8, at most --floor_history)")
    ap.add_argument("--decimate", type=int, default=None,
                    help="the recording is at the raw rate (float or int16): anti-alias FIR and decimation by this "
                         "factor (1 .. 64) ahead of the windows; --chunk then counts raw samples")
    ap.add_argument("--taps", default=None,
                    help="with --decimate: the FIR's taps, a .npy vector of at most 1025 (default: a Kaiser-windowed "
                         "sinc of 16 * D + 1 taps with its cut-off at 0.375 / D)")
    ap.add_argument("--common_mode", choices=["median", "mean"], default=None,
                    help="subtract the common mode -- per time sample the lower median or the mean over the fiber "
                         "-- from the stream the windows are cut from (with --decimate: after it); default: off")
    args = ap.parse_args()
    taps = None
    if args.taps is not None and args.decimate is None:
        ap.error("--taps needs --decimate")
    if args.decimate is not None:
        import numpy
        from mtl_das_pytorch_amd.data.resample import as_taps
        try:
            if args.taps is not None:
                taps = numpy.load(args.taps, allow_pickle=False)
            taps = as_taps(taps, args.decimate)
        except (ValueError, OSError) as e:
            ap.error(f"--decimate / --taps: {e}")
    noise_floor = args.noise_floor
    if args.gate_db is not None and args.chunk is not None and noise_floor == "auto":
        ap.error("--gate_db with --chunk needs --noise_floor running (or a power): 'auto' is the median over the "
                 "whole recording, which a growing one does not have")
    if noise_floor == "running":
        if args.chunk is None:
            ap.error("--noise_floor running is the floor of a growing recording: it needs --chunk")
        if args.floor_warmup is None:
            args.floor_warmup = min(8, args.floor_history)
        if not 1 <= args.floor_warmup <= args.floor_history <= 1024:
            ap.error("1 <= --floor_warmup <= --floor_history <= 1024")
    if noise_floor not in ("auto", "running"):
        try:
            noise_floor = float(noise_floor)
        except ValueError:
            ap.error("--noise_floor must be 'auto', 'running' or a power")
    if noise_floor != "auto" and args.gate_db is None:
        ap.error("--noise_floor needs --gate_db")

    from mtl_das_pytorch_amd import use_engine_graph_queues
    use_engine_graph_queues()  # before the first HIP call
    import numpy as np
    import torch
    from mtl_das_pytorch_amd.data.mat_dataset import load_mat
    from mtl_das_pytorch_amd.inference import WINDOW, predict_recording, prediction_map, window_starts
    from mtl_das_pytorch_amd.models import build_model
    from mtl_das_pytorch_amd.parallel.dist import init_distributed, shutdown

    stride = tuple(int(s) for s in args.stride.split(","))
    cell = tuple(int(s) for s in args.cell.split(",")) if args.cell else stride
    if args.map and (stride[0] > WINDOW[0] or stride[1] > WINDOW[1] or min(cell) < 1):
        # checked before the run, not after it: with a stride past the window some samples are in no window
        ap.error(f"--map needs windows that cover the recording: --stride at most {WINDOW[0]},{WINDOW[1]} "
                 "and a positive --cell")
    ctx = init_distributed()
    model = build_model(args.model, in_channels=args.in_channels)
    if args.model_path:
        model.load_state_dict(torch.load(args.model_path, map_location="cpu", weights_only=True), strict=True)
    use_engine = {"auto": None, "engine": True, "torch": False}[args.backend]
    live_maps = None
    if args.chunk is not None:
        if args.chunk < 1:
            ap.error("--chunk must be positive")
        if args.recording.endswith(".mat"):
            rec = np.asarray(load_mat(args.recording, (args.key,)), dtype=np.float32)
        else:
            rec = np.load(args.recording, mmap_mode="r", allow_pickle=False)
        if rec.dtype == np.int16 and args.decimate is None:
            ap.error("an int16 recording is at the raw rate: it needs --decimate")
        res, live_maps = live_run(model, args, rec, stride, cell if args.map else None, ctx, use_engine, noise_floor,
                                  taps)
    else:
        if args.recording.endswith(".mat"):
            rec = np.asarray(load_mat(args.recording, (args.key,)), dtype=np.float32)
        else:
            rec = np.load(args.recording, allow_pickle=False)
            if rec.dtype == np.int16 and args.decimate is None:
                ap.error("an int16 recording is at the raw rate: it needs --decimate")
            if rec.dtype != np.int16:  # int16 is uploaded as it is
                rec = rec.astype(np.float32)
        res = predict_recording(model, args.model, torch.from_numpy(rec), stride=stride, batch=args.batch_size,
                                ctx=ctx, use_engine=use_engine, gate_db=args.gate_db, noise_floor=noise_floor,
                                decimate=args.decimate, taps=taps, common_mode=args.common_mode)
    if ctx.is_main:
        import pandas as pd
        cols = {"fiber_start": res["positions"][:, 0], "time_start": res["positions"][:, 1]}
        for k in ("raw_time_start", "raw_time_stop", "distance_pred", "event_pred", "joint_pred", "power_db", "active"):
            if k in res:
                cols[k] = res[k].astype(np.int64) if k == "active" else res[k]
        pd.DataFrame(cols).to_csv(args.out, index=False)
        print(f"{len(res['positions'])} windows -> {args.out}")
        if args.map:
            shape = rec.shape[-2:]
            extra = {}
            if args.decimate is not None:  # the maps are the decimated recording's
                from mtl_das_pytorch_amd.data.resample import output_count
                shape = (shape[0], output_count(shape[1], len(taps), args.decimate))
            if live_maps is not None:
                maps = live_maps
            else:
                fs = window_starts(shape[0], WINDOW[0], stride[0])
                ts = window_starts(shape[1], WINDOW[1], stride[1])
                probs = res["joint_prob"] if "joint_prob" in res else np.concatenate(
                    [res[k] for k in ("distance_prob", "event_prob") if k in res], 1)
                if ctx.device.type == "cuda" and use_engine is not False:  # summed on the device; numpy fp64 otherwise
                    probs = torch.from_numpy(probs).to(ctx.device)
                maps = prediction_map(probs, fs, ts, shape, cell, active=res.get("active"))
            nfc, ntc = next(iter(maps.values())).shape[-2:]
            if args.decimate is not None:
                extra = {"time_edges_raw": np.minimum(np.arange(ntc + 1) * cell[1], shape[1]) * args.decimate,
                         "decimate": args.decimate, "taps": taps}
            if args.common_mode is not None:
                extra["common_mode"] = args.common_mode
            np.savez(args.map, fiber_edges=np.minimum(np.arange(nfc + 1) * cell[0], shape[0]),
                     time_edges=np.minimum(np.arange(ntc + 1) * cell[1], shape[1]), **extra, **maps)
            print(f"{nfc} x {ntc} cells -> {args.map}")
    shutdown(ctx)


def live_run(model, args, rec, stride, cell, ctx, use_engine, noise_floor="running", taps=None):
    """The recording through a LiveRecording, ``--chunk`` time samples at a time: the result dict of
    predict_recording (windows in its order) and, with ``cell``, the maps of prediction_map.  With ``--gate_db`` the
    live gate at ``noise_floor`` ("running" or a power).  With ``--decimate`` the chunks are raw (an int16 recording
    is pushed as int16) and the ring counts decimated samples.  With ``--common_mode`` the common mode is removed
    from every chunk on its way into the ring."""
    import numpy as np
    from mtl_das_pytorch_amd.inference import WINDOW, LiveRecording
    rec3 = rec if rec.ndim == 3 else rec[None]
    C, F, T = rec3.shape
    D = args.decimate or 1
    ring = args.ring if args.ring is not None else max(8 * WINDOW[1], WINDOW[1] + min(-(-args.chunk // D), 1 << 14))
    live = LiveRecording(model, args.model, F, C=C, stride=stride, cell=cell, ring=ring, batch=args.batch_size,
                         ctx=ctx, use_engine=use_engine, gate_db=args.gate_db,
                         noise_floor=noise_floor if args.gate_db is not None else "running",
                         floor_history=args.floor_history, floor_warmup=args.floor_warmup or 1,
                         decimate=args.decimate, taps=taps, common_mode=args.common_mode)
    dtype = np.int16 if (args.decimate is not None and rec3.dtype == np.int16) else np.float32
    outs = []
    for t in range(0, T, args.chunk):
        outs.append(live.push(np.ascontiguousarray(rec3[:, :, t:t + args.chunk], dtype=dtype)))
    outs.append(live.flush())
    live.close()
    pos = np.concatenate([o["positions"] for o in outs])
    if len(pos) == 0:
        raise ValueError(f"recording dimension {T} is shorter than the window {WINDOW[1]}"
                         + (f" times the decimation {D}" if args.decimate is not None else ""))
    order = np.lexsort((pos[:, 1], pos[:, 0]))  # fiber-major, as the whole-recording table
    res = {k: np.concatenate([o[k] for o in outs])[order] for k in outs[0] if k != "map_columns"}
    maps = None
    if cell is not None:
        maps = {k: np.concatenate([o["map_columns"][k] for o in outs], -1)
                for k in outs[0]["map_columns"] if k not in ("first", "last", "class_map")}
    return res, maps


if __name__ == "__main__":
    main()
