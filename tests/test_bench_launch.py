"""bench.py's launch contract without a launcher: ``--gpus 2`` with no WORLD_SIZE in the
environment starts its two rank processes itself (gloo on the CPU here; one rank per GPU on an MI355X node),
and exactly one JSON line -- rank 0's -- reaches stdout."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launches_two_ranks_and_prints_one_json_line():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = ""  # the CPU (gloo) form of the contract even on a GPU box
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    js = [l for l in lines if l.lstrip().startswith("{")]
    assert len(js) == 1, r.stdout  # (gloo itself prints its connection lines to stdout)
    out = json.loads(js[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 4
    assert out["value"] > 0 and out["dist_backend"] == "gloo"


def test_bench_self_launch_propagates_a_failing_rank():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--model", "nope"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and not r.stdout.strip()


def _bench_line(args, env, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    js = [l for l in r.stdout.splitlines() if l.lstrip().startswith("{")]
    assert len(js) == 1, r.stdout
    return json.loads(js[0])


def _check_dump(path, names):
    import numpy as np
    total = 0
    arrays = {}
    for n in names:
        a = np.load(os.path.join(path, n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), n
        total += a.nbytes
        arrays[n] = a
    assert sorted(os.listdir(path)) == sorted(n + ".npy" for n in names)
    assert total <= 64 * 2 ** 20
    return arrays


def test_bench_dump_outputs_and_step_count_on_the_cpu(tmp_path):
    """``--dump-outputs DIR`` writes the last timed step's outputs and the updated weights as float32 .npy files;
    ``--steps`` is the number of timed steps the line reports, with the time of one of them."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    d = str(tmp_path / "dump")
    out = _bench_line(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--dump-outputs", d], env)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]
    a = _check_dump(d, ["out0", "out1", "params"])
    assert a["out0"].shape[0] == 2 and a["out1"].shape[0] == 2


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs_and_full_adds_the_heldout_evaluation(tmp_path):
    """On the GPU: a plain run times its steps and writes the last step's outputs without the held-out evaluation;
    the same arguments give the same inputs, so a second run (here with ``--full``, which evaluates the held-out
    set after the outputs are written) dumps the same arrays up to the order of the kernels' float atomics."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    names = ["logp", "metrics", "params", "bn_mean", "bn_var"]
    args = ["--gpus", "1", "--steps", "3", "--warmup", "2"]
    d1, d2 = str(tmp_path / "plain"), str(tmp_path / "full")
    plain = _bench_line(args + ["--dump-outputs", d1], env)
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["dtype"] == "bf16"
    assert plain["heldout_acc_after_timed_steps"] is None and plain["heldout_samples"] == 0
    a = _check_dump(d1, names)
    assert a["logp"].shape[-2] == 32 and a["metrics"][0, 2] == 3 * 32  # 3 timed steps of 32 samples counted
    full = _bench_line(args + ["--full", "--heldout", "64", "--dump-outputs", d2], env)
    assert full["heldout_samples"] == 64 and 0.0 <= full["heldout_acc_after_timed_steps"]["event"] <= 1.0
    b = _check_dump(d2, names)
    for n in names:
        assert a[n].shape == b[n].shape
    # identical inputs, so the runs differ only by the order of float atomics.  Adam's first updates are +-lr
    # whatever the gradient's size, so a near-zero gradient whose sign the noise flips moves a weight 2 * lr apart
    # per step at the most: 5 steps at lr = 1e-3 / 1.5.  Log-probabilities (|x| of a few units) come from bf16
    # operands (eps 2^-8): a dozen eps.
    assert np.abs(a["params"] - b["params"]).max() <= 2 * 5 * 1e-3 / 1.5
    assert np.abs(a["logp"] - b["logp"]).max() < 0.05
