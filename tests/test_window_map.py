"""Event / distance maps of a recording (inference.prediction_map): the closed-form fp64 aggregation equals a
brute-force per-sample average, Model C's joint map is marginalised by decode_joint's coding, and the CLI."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a 23 x 41 recording, window (5, 8), stride (3, 5), cell (4, 7): the end-aligned last window (18 after 15; 33 after
# 30) and the ragged last cell (rows 20..22; times 35..40) are both present
SHAPE, WIN, STRIDE, CELL = (23, 41), (5, 8), (3, 5), (4, 7)


def _geometry():
    from mtl_das_pytorch_amd.inference import window_starts
    fs, ts = window_starts(SHAPE[0], WIN[0], STRIDE[0]), window_starts(SHAPE[1], WIN[1], STRIDE[1])
    assert list(fs) == [0, 3, 6, 9, 12, 15, 18] and list(ts) == [0, 5, 10, 15, 20, 25, 30, 33]
    return fs, ts


def _brute_force(probs, fs, ts, K):
    """Paint every window's probability over its samples, average per sample, then average per cell."""
    acc = np.zeros((K,) + SHAPE)
    cnt = np.zeros(SHAPE)
    for a, f0 in enumerate(fs):
        for b, t0 in enumerate(ts):
            acc[:, f0:f0 + WIN[0], t0:t0 + WIN[1]] += probs[a * len(ts) + b][:, None, None]
            cnt[f0:f0 + WIN[0], t0:t0 + WIN[1]] += 1
    assert (cnt > 0).all() and cnt.min() < cnt.max()  # samples differ in how many windows cover them
    sample = acc / cnt
    nfc, ntc = -(-SHAPE[0] // CELL[0]), -(-SHAPE[1] // CELL[1])
    out = np.zeros((K, nfc, ntc))
    for i in range(nfc):
        for j in range(ntc):
            out[:, i, j] = sample[:, i * CELL[0]:(i + 1) * CELL[0], j * CELL[1]:(j + 1) * CELL[1]].mean((1, 2))
    return out


def test_map_reference_equals_brute_force():
    from mtl_das_pytorch_amd.inference import window_map_reference
    fs, ts = _geometry()
    K = 3
    probs = np.random.default_rng(0).random((len(fs) * len(ts), K))
    want = _brute_force(probs, fs, ts, K)
    assert want.shape == (K, 6, 6)
    got = window_map_reference(probs, fs, ts, SHAPE, CELL, WIN)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-12
    # a constant probability maps to itself, whatever the overlaps
    const = window_map_reference(np.full((len(fs) * len(ts), 1), 0.25), fs, ts, SHAPE, CELL, WIN)
    assert np.abs(const - 0.25).max() < 1e-12


def test_map_reference_rejects_starts_with_a_gap():
    import pytest
    from mtl_das_pytorch_amd.inference import window_map_reference
    _, ts = _geometry()
    with pytest.raises(ValueError):  # rows 5..8 are in no window
        window_map_reference(np.zeros((5 * len(ts), 1)), [0, 9, 12, 15, 18], ts, SHAPE, CELL, WIN)


def test_prediction_map_tasks_and_joint_marginals():
    from mtl_das_pytorch_amd.inference import prediction_map, window_map_reference
    fs, ts = _geometry()
    rng = np.random.default_rng(1)
    n = len(fs) * len(ts)
    joint = rng.random((n, 32))
    joint /= joint.sum(1, keepdims=True)
    m = prediction_map({"joint_prob": joint}, fs, ts, SHAPE, CELL, WIN)
    full = window_map_reference(joint, fs, ts, SHAPE, CELL, WIN)
    assert m["event_map"].shape == (2, 6, 6) and m["distance_map"].shape == (16, 6, 6)
    assert m["distance_mean_m"].shape == (6, 6)
    # joint = distance + 16 * event
    assert np.allclose(m["event_map"][1], full[16:].sum(0), atol=1e-12)
    assert np.allclose(m["distance_map"][3], full[3] + full[19], atol=1e-12)
    assert np.allclose(m["event_map"].sum(0), 1, atol=1e-12) and np.allclose(m["distance_map"].sum(0), 1, atol=1e-12)
    d, e = joint.reshape(n, 2, 16).sum(1), joint.reshape(n, 2, 16).sum(2)
    ab = prediction_map({"distance_prob": d, "event_prob": e}, fs, ts, SHAPE, CELL, WIN)
    tab = prediction_map(torch.from_numpy(np.concatenate([d, e], 1)), fs, ts, SHAPE, CELL, WIN)
    for k in ("event_map", "distance_map", "distance_mean_m"):
        assert np.allclose(ab[k], m[k], atol=1e-12) and np.array_equal(ab[k], tab[k])
    assert np.allclose(m["distance_mean_m"], np.tensordot(np.arange(16.0), m["distance_map"], 1))


def test_infer_cli_map(tmp_path):
    rec = np.random.default_rng(0).standard_normal((150, 500)).astype(np.float32)
    np.save(tmp_path / "rec.npy", rec)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--model", "MTL", "--backend", "torch",
                        "--recording", str(tmp_path / "rec.npy"), "--stride", "50,125", "--cell", "40,100",
                        "--out", str(tmp_path / "p.csv"), "--map", str(tmp_path / "m.npz")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(tmp_path / "m.npz")
    nfc, ntc = 4, 5  # ceil(150 / 40), ceil(500 / 100)
    assert z["event_map"].shape == (2, nfc, ntc) and z["distance_map"].shape == (16, nfc, ntc)
    assert z["distance_mean_m"].shape == (nfc, ntc)
    assert list(z["fiber_edges"]) == [0, 40, 80, 120, 150] and list(z["time_edges"]) == [0, 100, 200, 300, 400, 500]
    assert np.abs(z["event_map"].sum(0) - 1).max() < 1e-6
    assert np.abs(z["distance_map"].sum(0) - 1).max() < 1e-6
    import pandas as pd
    assert len(pd.read_csv(tmp_path / "p.csv")) == 2 * 3  # the CSV is what it was: fiber starts 0, 50; time starts 0, 125, 250


def test_infer_cli_map_refuses_a_stride_past_the_window_before_the_run(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--model", "MTL", "--backend", "torch",
                        "--recording", str(tmp_path / "missing.npy"), "--stride", "120,125",
                        "--out", str(tmp_path / "p.csv"), "--map", str(tmp_path / "m.npz")],
                       env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 2 and "--map needs windows that cover the recording" in r.stderr
    assert not (tmp_path / "p.csv").exists()
