"""Bitwise digest of a few captured training steps, for comparing two builds of the HIP extension.

    python tools/ext_digest.py [--model MTL|multi_classifier|...] [--steps 5] [--snr lo,hi [--noise-seed N]]
    MDA_EXT_PATH=ab/_mda_hip_base.so python tools/ext_digest.py ...

Builds the model's program from the shipped tuned table (no measuring, so both builds run the same kernel
configurations), trains ``--steps`` graph-replayed steps on a fixed synthetic batch schedule and prints the
sha256 of the fp32 master weights, gradients, Adam moments and BN running statistics, and of the head's
correct / count metric columns, with the number of arrays and bytes hashed.  ``--snr lo,hi``: the steps train on
noisy inputs (StepRunner.set_train_noise), so the digest also covers the noisy gather.
Kernel changes that only reorder loads (no arithmetic change) must print the same digest as the baseline build.
"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="MTL")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--snr", type=str, default=None, metavar="LO,HI", help="train with on-device SNR noise (dB)")
    ap.add_argument("--noise-seed", type=int, default=1)
    args = ap.parse_args()
    from mtl_das_pytorch_amd import use_engine_graph_queues
    use_engine_graph_queues()
    import torch
    from mtl_das_pytorch_amd.data.synthetic import generate
    from mtl_das_pytorch_amd.engine.inception import InceptionProgram
    from mtl_das_pytorch_amd.engine.mtl import MTLProgram
    from mtl_das_pytorch_amd.engine.step import StepRunner
    from mtl_das_pytorch_amd.engine.tune import autotune_program
    from mtl_das_pytorch_amd.models import build_model, encode_joint
    from mtl_das_pytorch_amd.ops import hip

    hip.lib()
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = build_model(args.model)
    joint = args.model == "multi_classifier"
    prog = (InceptionProgram(model, args.batch, dev) if joint else MTLProgram(model, args.batch, dev))
    prog.set_optimizer(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    prog.segment_backward(1)
    autotune_program(prog, measure=False)
    n = 4 * args.batch
    X, d, e = generate(n, seed=1000, device=dev)
    labels = encode_joint(d, e) if joint else torch.stack([d, e], 1)
    runner = StepRunner(prog, X, labels, use_graph=True)
    runner.set_lr(1e-3 / 1.5)
    g = torch.Generator().manual_seed(7)
    sched = torch.stack([torch.randperm(n, generator=g)[:args.batch] for _ in range(args.steps)]).to(dev)
    runner.set_index_schedule(sched)
    if args.snr is not None:
        from mtl_das_pytorch_amd.data.noise import parse_snr_range
        runner.set_train_noise(parse_snr_range(args.snr), seed=args.noise_seed)
    for _ in range(args.steps):
        runner.train_step()
    torch.cuda.synchronize()
    f = prog.flat
    h = hashlib.sha256()
    arrays = nbytes = 0
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_mean", "bn_var"):
        t = getattr(f, name, None)
        if t is not None:
            raw = t.detach().cpu().numpy().tobytes()
            h.update(raw)
            arrays, nbytes = arrays + 1, nbytes + len(raw)
    # the metric rows' correct / count columns (the loss column is an fp32 atomic sum: its last bits follow the
    # order the blocks arrive in, run to run)
    raw = prog.metrics[:, 1:3].detach().cpu().numpy().tobytes()
    hm = hashlib.sha256(raw)
    print(f"DIGEST {args.model} steps={args.steps} state={h.hexdigest()[:16]} metrics={hm.hexdigest()[:16]} "
          f"ext={os.environ.get('MDA_EXT_PATH', 'in-tree')} snr={args.snr} arrays={arrays + 1} "
          f"bytes={nbytes + len(raw)}", flush=True)
    runner.close()


if __name__ == "__main__":
    main()
