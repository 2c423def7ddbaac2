"""The activity gate of recording inference on the CPU: the torch backend of predict_recording(gate_db=...) against
the fp64 flags, the "auto" noise floor, prediction_map(active=...) against an fp64 ratio written out here, and the
command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_model = {}


def _model_a():
    """Model A, the count of windows its forward has seen, and the ungated result on the fixture (computed once)."""
    if not _model:
        from mtl_das_pytorch_amd.inference import predict_recording
        from mtl_das_pytorch_amd.models import build_model
        torch.manual_seed(0)
        m = build_model("MTL").eval()
        seen = [0]
        forward = m.forward

        def counted(x):
            seen[0] += len(x)
            return forward(x)

        m.forward = counted
        rec = torch.from_numpy(G.fixture()[0].copy())
        _model.update(m=m, seen=seen, rec=rec,
                      plain=predict_recording(m, "MTL", rec, stride=G.STRIDE, batch=35, use_engine=False))
        assert seen[0] == 140
    return _model


@pytest.mark.parametrize("noise_floor", [1.0, "auto"])
def test_torch_backend_evaluates_only_active_windows(noise_floor):
    from mtl_das_pytorch_amd.inference import predict_recording
    want = G.fixture_flags(noise_floor)
    assert want.sum() == 60  # both floors, computed in fp64 when the fixture was chosen
    s = _model_a()
    s["seen"][0] = 0
    res = predict_recording(s["m"], "MTL", s["rec"], stride=G.STRIDE, batch=35, use_engine=False, gate_db=G.GATE_DB,
                            noise_floor=noise_floor)
    assert s["seen"][0] == want.sum()  # the model never saw a quiet window
    assert res["active"].dtype == bool and np.array_equal(res["active"], want)
    power = G.fixture()[3]
    assert np.allclose(res["power_db"], 10 * np.log10(power), rtol=0, atol=1e-9)
    assert set(res) == set(s["plain"]) | {"active", "power_db"}
    for k in ("distance", "event"):
        assert (res[f"{k}_pred"][~want] == -1).all() and (res[f"{k}_prob"][~want] == 0).all()
        assert np.array_equal(res[f"{k}_pred"][want], s["plain"][f"{k}_pred"][want])
        assert np.array_equal(res[f"{k}_prob"][want], s["plain"][f"{k}_prob"][want])
    assert np.array_equal(res["positions"], s["plain"]["positions"])


class _Rank:
    """A data-parallel context of two ranks whose all-reduce is left to the test (the shards' sum)."""
    enabled, world, device = True, 2, torch.device("cpu")

    def __init__(self, rank):
        self.rank = rank

    def all_reduce_(self, t):
        pass


def test_every_rank_has_all_flags_and_gates_its_own_shard():
    from mtl_das_pytorch_amd.inference import predict_recording
    want = G.fixture_flags(1.0)
    s = _model_a()
    parts = []
    for rank in range(2):
        s["seen"][0] = 0
        res = predict_recording(s["m"], "MTL", s["rec"], stride=G.STRIDE, batch=35, ctx=_Rank(rank),
                                use_engine=False, gate_db=G.GATE_DB, noise_floor=1.0)
        assert np.array_equal(res["active"], want)  # all 140 flags on every rank
        assert s["seen"][0] == want[70 * rank:70 * (rank + 1)].sum()  # the model saw the shard's active windows
        parts.append(res["event_prob"])
    assert (parts[0][70:] == 0).all() and (parts[1][:70] == 0).all()
    assert np.array_equal((parts[0] + parts[1])[want], s["plain"]["event_prob"][want])


def test_joint_model_decodes_quiet_windows_to_minus_one():
    """Model C's distance_pred / event_pred are decoded from the joint prediction: quiet windows are -1 there too.
    A (100, 600) recording with a loud second half: 1 x 5 windows."""
    from mtl_das_pytorch_amd.inference import predict_recording
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(0)
    m = build_model("multi_classifier").eval()
    rec = np.random.default_rng(1).standard_normal((100, 600)).astype(np.float32)
    rec[:, 350:] *= 4
    res = predict_recording(m, "multi_classifier", torch.from_numpy(rec), stride=(100, 100), batch=8,
                            use_engine=False, gate_db=6.0, noise_floor=1.0)
    assert res["active"].tolist() == [False, False, True, True, True]  # starts 0, 100, 200, 300, 350
    for k in ("joint_pred", "distance_pred", "event_pred"):
        assert (res[k][:2] == -1).all() and (res[k][2:] >= 0).all(), k
    assert (res["joint_prob"][:2] == 0).all() and np.allclose(res["joint_prob"][2:].sum(1), 1, atol=1e-5)


def test_auto_floor_is_the_lower_median_per_fiber_start():
    from mtl_das_pytorch_amd.inference import active_reference, noise_floor_reference
    _, fs, ts, power = G.fixture()
    floor = noise_floor_reference(power, len(ts), "auto")
    assert floor.shape == (len(fs),) and np.array_equal(floor, G.lower_median(power, len(ts)))
    # an even count takes the lower of the two middle values: (nt - 1) // 2 = 4 of 10
    assert floor[0] == np.sort(power[:10])[4]
    assert np.array_equal(noise_floor_reference(power, len(ts), 2.5), np.full(len(fs), 2.5))
    assert np.array_equal(active_reference(power, len(ts), G.GATE_DB, "auto"), G.fixture_flags("auto"))
    p = power.copy()
    p[3] = np.nan  # a NaN power is never hidden
    assert active_reference(p, len(ts), 60.0, 1.0).tolist() == [n == 3 for n in range(140)]


def test_window_power_reference_is_the_centred_mean_square():
    from mtl_das_pytorch_amd.inference import window_power_reference
    rng = np.random.default_rng(2)
    rec = rng.standard_normal((2, 9, 11)) + np.array([50.0, -20.0])[:, None, None]
    p = window_power_reference(rec, [0, 4], [0, 3, 5], (5, 6))
    assert p.shape == (6,)
    w = rec[:, 4:9, 3:9]
    want = np.mean([np.var(w[0]), np.var(w[1])])  # per channel around its own mean, then the channels' mean
    assert abs(p[1 * 3 + 1] - want) <= 1e-12 * want


def test_prediction_map_with_flags_is_the_ratio_of_weighted_sums():
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map
    from mtl_das_pytorch_amd.ops.functional import window_cell_weights
    _, fs, ts, _ = G.fixture()
    shape, cell = (230, 700), (20, 100)
    rng = np.random.default_rng(3)
    active = rng.random(140) < 0.5
    active.reshape(14, 10)[:, :4] = False  # times 0 .. 200 are covered by these windows only (starts 0 .. 150)
    probs = rng.random((140, 18)).astype(np.float32)
    probs[~active] = 0
    got = prediction_map(probs, fs, ts, shape, cell, active=active)
    wf = window_cell_weights(fs, WINDOW[0], shape[0], cell[0])
    wt = window_cell_weights(ts, WINDOW[1], shape[1], cell[1])
    f = active.reshape(14, 10).astype(np.float64)
    act = np.einsum("ai,bj,ab->ij", wf, wt, f)
    num = np.einsum("ai,bj,abk->kij", wf, wt, probs.astype(np.float64).reshape(14, 10, 18))
    assert got["activity_map"].shape == (12, 7) and np.allclose(got["activity_map"], act, rtol=1e-12, atol=0)
    empty = act == 0
    assert empty[:, :2].all() and not empty[:, 2:].all()  # the cells of times 0 .. 200 hear nothing
    with np.errstate(invalid="ignore", divide="ignore"):
        want = num / act
    for k, rows in (("distance_map", slice(0, 16)), ("event_map", slice(16, 18))):
        assert np.array_equal(np.isnan(got[k]), np.broadcast_to(empty, got[k].shape)), k
        assert np.allclose(got[k][:, ~empty], want[rows][:, ~empty], rtol=1e-12, atol=0), k
    assert np.array_equal(np.isnan(got["distance_mean_m"]), empty)
    # a result dict that carries its flags needs no argument; without flags nothing changes
    res = {"distance_prob": probs[:, :16], "event_prob": probs[:, 16:], "active": active}
    again = prediction_map(res, fs, ts, shape, cell)
    assert np.array_equal(again["event_map"], got["event_map"], equal_nan=True)
    assert "activity_map" not in prediction_map(probs, fs, ts, shape, cell)


def _infer(tmp_path, *extra):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--model", "MTL", "--recording",
                           str(tmp_path / "rec.npy"), "--out", str(tmp_path / "p.csv"), *extra], env=env,
                          capture_output=True, text=True, timeout=600)


def test_infer_cli_gate(tmp_path):
    rec = np.random.default_rng(0).standard_normal((100, 600)).astype(np.float32)
    rec[:, 350:] *= 4
    np.save(tmp_path / "rec.npy", rec)
    r = _infer(tmp_path, "--gate_db", "3", "--chunk", "200")
    assert r.returncode == 2 and "--chunk" in r.stderr and not (tmp_path / "p.csv").exists()
    r = _infer(tmp_path, "--gate_db", "6", "--noise_floor", "1.0", "--stride", "100,100", "--map",
               str(tmp_path / "m.npz"))
    assert r.returncode == 0, r.stderr[-2000:]
    import pandas as pd
    df = pd.read_csv(tmp_path / "p.csv")
    assert len(df) == 5 and {"power_db", "active", "distance_pred", "event_pred"} <= set(df.columns)
    assert df["active"].tolist() == [0, 0, 1, 1, 1]
    assert (df["event_pred"][:2] == -1).all() and (df["event_pred"][2:] >= 0).all()
    assert df["power_db"][0] < 1 < 6 < df["power_db"][4]
    maps = np.load(tmp_path / "m.npz")
    act = maps["activity_map"]
    assert act.shape == (1, 6) and act[0, 0] == 0 and abs(act[0, 5] - 1) < 1e-12
    assert np.isnan(maps["event_map"][:, 0, 0]).all() and not np.isnan(maps["event_map"][:, 0, 5]).any()
