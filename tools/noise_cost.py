#!/usr/bin/env python3
"""What the on-device SNR augmentation costs a training step: replays of the captured ``train_full`` graph of one
program with the noise off and on (two runners over the same program and resident set, schedule form as the trainer
runs it), alternating rounds, device-event timed; then the two gather kernels in isolation (back-to-back launches
on one stream, the step's own arguments).  Prints one JSON line.

    python tools/noise_cost.py [MTL|single_event|...] [--steps 300] [--rounds 3] [--snr 0,20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtl_das_pytorch_amd.data.noise import parse_snr_range  # noqa: E402
from mtl_das_pytorch_amd.data.synthetic import generate  # noqa: E402
from mtl_das_pytorch_amd.engine.mtl import MTLProgram  # noqa: E402
from mtl_das_pytorch_amd.engine.step import StepRunner  # noqa: E402
from mtl_das_pytorch_amd.engine.tune import autotune_program  # noqa: E402
from mtl_das_pytorch_amd.models import build_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="MTL")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--snr", type=str, default="0,20")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=4096)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(1234)
    B = args.batch
    p = MTLProgram(build_model(args.model), B, "cuda")
    p.set_optimizer(weight_decay=1e-5)
    autotune_program(p, measure=False)
    X, d, e = generate(args.samples, seed=1, device="cuda")
    labels = torch.stack([d, e], 1)
    sched = torch.randperm(args.samples, device="cuda")[:args.samples // B * B].view(-1, B)
    runners = {}
    for name in ("off", "on"):
        r = runners[name] = StepRunner(p, X, labels, use_graph=True)
        r.set_lr(1e-3)
        r.set_index_schedule(sched)
        if name == "on":
            r.set_train_noise(parse_snr_range(args.snr), seed=1)
        for _ in range(20):  # warm-up: capture + first replays
            r.train_step()
    torch.cuda.synchronize()

    def timed(fn, n) -> float:
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        t.record()
        torch.cuda.synchronize()
        return 1e3 * s.elapsed_time(t) / n  # us

    step = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            step[name].append(timed(runners[name].graphs["train_full"].replay, args.steps))
    # the gather launches alone, with the step's arguments (clear included)
    gather = {"off": [], "on": []}
    phases = {n: p.gather_phase(X, labels, r.schedule, clear=True, cursor=r.cursor, noise=r._noise_spec("train"))
              for n, r in runners.items()}
    launches = {n: [l for l in ph.launches if l.name.startswith("gather")][0] for n, ph in phases.items()}
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(args.rounds):
        for name in ("off", "on"):
            timed(lambda: launches[name](st), 20)
            gather[name].append(timed(lambda: launches[name](st), args.steps))
    out = {"model": args.model, "batch": B, "snr": args.snr, "replays_per_run": args.steps,
           "step_us": {k: [round(v, 1) for v in vs] for k, vs in step.items()},
           "gather_kernel_us": {k: [round(v, 2) for v in vs] for k, vs in gather.items()}}
    print(json.dumps(out), flush=True)
    for r in runners.values():
        r.close()


if __name__ == "__main__":
    main()
