"""CPU: common-mode removal -- the definition (data/common_mode.py) against np.median, math.fsum and an explicit
loop, its NaN / inf / signed-zero / tie conventions, the torch backends of predict_recording(common_mode=...) and
LiveRecording(common_mode=...) against the definition applied beforehand, the gate fixture the stage exists for,
the argument errors and infer.py --common_mode."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOWS = ("median", "mean")
STRIDE, CELL, CHUNKS = (100, 125), (50, 125), (1, 249, 130, 77, 443)
GATE = dict(gate_db=3.0, noise_floor=1.0)
_cache = {}


def _ref(x, how):
    from mtl_das_pytorch_amd.data.common_mode import common_mode_reference
    return common_mode_reference(x, how)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the definition ---------------------------------------------------------------------------------------------
def test_median_is_np_median_for_odd_F_and_the_lower_middle_for_even_F():
    rng = np.random.default_rng(0)
    for Fn in (1, 3, 5, 101):
        x = rng.standard_normal((2, Fn, 17)).astype(np.float32)
        y, m = _ref(x, "median")
        assert y.dtype == m.dtype == np.float32 and y.shape == x.shape and m.shape == (2, 17)
        assert np.array_equal(m, np.median(x, axis=1))
        assert np.array_equal(_bits(y), _bits(x - m[:, None, :]))
    assert not _ref(rng.standard_normal((1, 1, 9)), "median")[0].any()  # F = 1: all zeros
    for Fn in (2, 4, 100):
        x = rng.standard_normal((2, Fn, 17)).astype(np.float32)
        m = _ref(x, "median")[1]
        s = np.sort(x, axis=1)
        assert np.array_equal(m, s[:, Fn // 2 - 1]) and (m < s[:, Fn // 2]).all()
    # [F, T] is one channel
    x = rng.standard_normal((6, 5)).astype(np.float32)
    y2, m2 = _ref(x, "median")
    assert y2.shape == (1, 6, 5) and np.array_equal(m2[0], np.sort(x, 0)[2])


def test_median_nan_sorts_last():
    x = np.arange(10, dtype=np.float32).reshape(1, 10, 1).repeat(3, 2).copy()
    x[0, [0, 3, 7, 9], 0] = np.nan                 # 4 of 10: the finite ones are 1 2 4 5 6 8, rank 4 is 6
    x[0, [0, 1, 2, 3, 4, 5], 1] = np.nan           # 6 of 10: the median is NaN
    x[0, [1, 2, 3, 4, 5], 2] = -np.nan             # 5 of 10 (sign set): rank 4 is the largest finite one, 9
    y, m = _ref(x, "median")
    assert m[0, 0] == 6 and np.isnan(m[0, 1]) and m[0, 2] == 9
    assert np.array_equal(np.isnan(y[0, :, 0]), np.isnan(x[0, :, 0])) and np.isnan(y[0, :, 1]).all()
    fin = ~np.isnan(x[0, :, 0])
    assert np.array_equal(y[0, fin, 0], x[0, fin, 0] - 6)


def test_median_inf_signed_zeros_and_ties():
    inf = np.inf
    x = np.array([[-inf, 1, 2, inf, inf], [-inf, -inf, -inf, 0, 1], [3, inf, inf, inf, -1]], dtype=np.float32).T[None]
    y, m = _ref(x, "median")
    assert m[0].tolist() == [2, -inf, inf]
    assert y[0, :, 0].tolist() == [-inf, -1, 0, inf, inf]
    assert np.isnan(y[0, :3, 1]).all() and y[0, 3:, 1].tolist() == [inf, inf]   # -inf - -inf is NaN
    assert y[0, 0, 2] == -inf and np.isnan(y[0, 1:4, 2]).all()
    # zeros of both signs: the median is +0.0 by bits, whichever zero the sort leaves in the middle
    z = np.array([[-0.0, 0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0], [-1.0, -0.0, 1.0]], dtype=np.float32).T[None]
    yz, mz = _ref(z, "median")
    assert (_bits(mz) == 0).all()
    assert np.array_equal(_bits(yz), _bits(z - np.float32(0.0)))
    # heavy ties
    rng = np.random.default_rng(1)
    t = rng.integers(-2, 3, (2, 64, 40)).astype(np.float32)
    mt = _ref(t, "median")[1]
    assert np.array_equal(mt, np.sort(t, 1)[:, 31]) and ((t <= mt[:, None]).sum(1) >= 32).all()
    c = np.full((1, 7, 3), 2.5, dtype=np.float32)
    assert not _ref(c, "median")[0].any() and (_ref(c, "median")[1] == 2.5).all()


def test_mean_is_the_ordered_fp64_sum():
    rng = np.random.default_rng(2)
    Fn = 300
    x = (rng.standard_normal((2, Fn, 5)) * 10.0 ** rng.integers(-3, 4, (2, Fn, 5))).astype(np.float32)
    y, m = _ref(x, "mean")
    assert y.dtype == m.dtype == np.float32 and m.shape == (2, 5)
    for c in range(2):
        for t in range(5):
            col = [float(v) for v in x[c, :, t]]
            acc = 0.0
            for v in col:
                acc += v
            assert m[c, t] == np.float32(acc / Fn)  # exactly the explicit loop
            # Fn additions, each within 2^-53 of a partial sum that is at most sum |x|
            assert abs(acc - math.fsum(col)) <= Fn * 2.0 ** -53 * math.fsum(abs(v) for v in col)
    assert np.array_equal(_bits(y), _bits(x - m[:, None, :]))
    # an order that matters: pairwise summation gives 0 here, the definition's order 2^-30
    z = np.array([1.0, 2.0 ** -60, -1.0, 2.0 ** -30], dtype=np.float32).reshape(1, 4, 1)
    assert _ref(z, "mean")[1][0, 0] == np.float32(2.0 ** -30 / 4)
    assert _ref(np.ones((1, 1, 3), np.float32), "mean")[0].tolist() == [[[0.0, 0.0, 0.0]]]


def test_as_common_mode():
    from mtl_das_pytorch_amd.data.common_mode import as_common_mode
    assert as_common_mode(None) is None and as_common_mode("median") == "median" and as_common_mode("mean") == "mean"
    for bad in ("Median", "mode", "", 0, True, ["median"]):
        with pytest.raises(ValueError):
            as_common_mode(bad)
    with pytest.raises(ValueError):
        _ref(np.zeros((1, 2, 3)), None)
    with pytest.raises(ValueError):
        _ref(np.zeros((1, 2, 3)), "max")


# ---- the torch backends -------------------------------------------------------------------------------------------
def _model():
    from mtl_das_pytorch_amd.models import build_model
    if "m" not in _cache:
        torch.manual_seed(0)
        m = build_model("MTL")
        m.train()  # non-trivial BN running statistics
        with torch.no_grad():
            m(torch.randn(4, 1, 100, 250))
        _cache["m"] = m.eval()
    return _cache["m"]


def _fixture():
    """The 200 x 900 recording the stage exists for: unit-variance noise, an event (x 6) on fibers 100-199 from
    t = 500, and a common-mode burst 5 randn on every fiber for t in [200, 450).  (burst-free, recorded)."""
    if "fix" not in _cache:
        g = torch.Generator().manual_seed(3)
        clean = torch.randn(200, 900, generator=g)
        clean[100:, 500:] *= 6.0
        rec = clean.clone()
        rec[:, 200:450] += 5.0 * torch.randn(250, generator=g)
        _cache["fix"] = (clean, rec)
    return _cache["fix"]


def _predict(rec, **kw):
    from mtl_das_pytorch_amd.inference import predict_recording
    return predict_recording(_model(), "MTL", rec, stride=STRIDE, batch=8, use_engine=False, **kw)


@pytest.mark.parametrize("how", HOWS)
def test_predict_recording_is_predict_recording_on_the_cleaned_recording(how):
    from mtl_das_pytorch_amd.inference import decimate_recording, remove_common_mode
    _, rec = _fixture()
    clean, trace = remove_common_mode(rec, how, use_engine=False)
    want_y, want_m = _ref(rec.numpy(), how)
    assert clean.dtype == torch.float32 and clean.shape == (1, 200, 900) and trace.shape == (1, 900)
    assert np.array_equal(_bits(clean.numpy()), _bits(want_y)) and np.array_equal(_bits(trace.numpy()), _bits(want_m))
    got, want = _predict(rec, common_mode=how, **GATE), _predict(torch.from_numpy(want_y), **GATE)
    assert set(got) == set(want) and "active" in got
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # with decimation the stage runs on the decimated recording
    raw = torch.randn(100, 3 * 299 + 49, generator=torch.Generator().manual_seed(4))
    raw[:, 300:600] += 4.0 * torch.randn(300, generator=torch.Generator().manual_seed(5))
    dec = decimate_recording(raw, 3, use_engine=False)
    got = _predict(raw, decimate=3, common_mode=how)
    want = _predict(torch.from_numpy(_ref(dec.numpy(), how)[0]))
    assert "raw_time_start" in got
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _live(chunks, sizes, ring=512, **kw):
    from mtl_das_pytorch_amd.inference import LiveRecording
    live = LiveRecording(_model(), "MTL", chunks.shape[0], stride=STRIDE, cell=CELL, ring=ring, batch=8,
                         use_engine=False, **kw)
    outs, at = [], 0
    for n in sizes:
        outs.append(live.push(chunks[:, at:at + n]))
        at += n
    assert at == chunks.shape[1] and live.captures == 0
    outs.append(live.flush())
    ring_now, total = live.backend.ring.clone(), live.total
    live.close()
    return outs, ring_now, total


def _same_windows(outs, off):
    pos = np.concatenate([o["positions"] for o in outs])
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    assert np.array_equal(pos[order], off["positions"])
    for k in ("distance_pred", "event_pred"):
        assert np.array_equal(np.concatenate([o[k] for o in outs])[order], off[k]), k
    for k in ("distance_prob", "event_prob"):
        # the fp32 module on other batches of the same windows: the tolerance of the decimated live test
        err = np.abs(np.concatenate([o[k] for o in outs])[order].astype(np.float64) - off[k]).max()
        print(f"torch live (common mode) vs offline {k}: max abs diff {err:.3e}")
        assert err <= 1e-5, (k, err)


@pytest.mark.parametrize("how", HOWS)
def test_torch_live_matches_predict_recording(how):
    """The ring holds exactly the definition's bits of the stream's last columns however it was cut; windows,
    predictions and probabilities are the offline run's."""
    _, rec = _fixture()
    outs, ring, total = _live(rec, CHUNKS, common_mode=how)
    assert total == 900
    want = _ref(rec.numpy(), how)[0]
    cols = np.arange(900 - 512, 900)
    assert np.array_equal(_bits(ring.numpy()[:, :, cols % 512]), _bits(want[:, :, cols]))
    _same_windows(outs, _predict(rec, common_mode=how))
    # the raw stream: decimated piece by piece, each piece cleaned
    raw = torch.randn(100, 3 * 899 + 49, generator=torch.Generator().manual_seed(6))
    raw[:, 900:1500] += 4.0 * torch.randn(600, generator=torch.Generator().manual_seed(7))
    outs, _, total = _live(raw, (1, 747, 390, 231, 1377), decimate=3, common_mode=how)
    assert total == 900
    _same_windows(outs, _predict(raw, decimate=3, common_mode=how))


def test_the_stage_closes_the_gate_the_burst_opened():
    """The issue's numbers: the burst opens the gate on 11 of 14 windows; after either estimate the flags are the
    burst-free recording's, 4 of 14; the cleaned quiet powers stay at or below 1.08 against a threshold of
    10^0.3 = 1.995 and the weakest active window has power 18.2, so the flags do not hang on a rounding.  (Both
    figures are the mean's, the worse of the two, at the issue's digits: 1.0824 -- the mean over a fiber half of
    which carries the event keeps (36 + 1) / 2 / 200 of variance -- and 18.21; the median's are 1.0076 and 18.29.)"""
    from mtl_das_pytorch_amd.inference import WINDOW, active_reference, window_power_reference, window_starts
    clean, rec = _fixture()
    fs, ts = window_starts(200, WINDOW[0], STRIDE[0]), window_starts(900, WINDOW[1], STRIDE[1])
    assert len(fs) * len(ts) == 14
    flags = lambda x: active_reference(window_power_reference(x, fs, ts), len(ts), **GATE)
    want = flags(clean)
    assert want.sum() == 4 and flags(rec).sum() == 11
    res = {None: _predict(rec, **GATE), "free": _predict(clean, **GATE)}
    assert res[None]["active"].sum() == 11 and np.array_equal(res["free"]["active"], want)
    for how in HOWS:
        y = _ref(rec.numpy(), how)[0]
        power = window_power_reference(y, fs, ts)
        print(f"{how}: quiet powers up to {power[~want].max():.4f}, weakest active {power[want].min():.2f}")
        assert np.array_equal(flags(y), want)
        # the issue's figures to the digits it gives: 1.0076 / 18.29 (median), 1.0824 / 18.21 (mean)
        assert round(float(power[~want].max()), 2) <= 1.08 and power[want].min() >= 18.2
        got = _predict(rec, common_mode=how, **GATE)
        assert np.array_equal(got["active"], want) and got["active"].sum() == 4
        assert (got["distance_pred"][~want] == -1).all()


def test_argument_errors():
    from mtl_das_pytorch_amd.inference import LiveRecording, predict_recording, remove_common_mode
    m = _model()
    rec = torch.zeros(100, 300)
    for bad in ("max", "Median", 1):
        with pytest.raises(ValueError):
            predict_recording(m, "MTL", rec, use_engine=False, common_mode=bad)
        with pytest.raises(ValueError):
            LiveRecording(m, "MTL", 100, use_engine=False, common_mode=bad)
        with pytest.raises(ValueError):
            remove_common_mode(rec, bad, use_engine=False)
    with pytest.raises(ValueError):
        remove_common_mode(rec, None, use_engine=False)
    # int16 is the raw rate's type: without decimate it stays an error
    raw = torch.zeros(100, 300, dtype=torch.int16)
    with pytest.raises(ValueError, match="int16"):
        predict_recording(m, "MTL", raw, use_engine=False, common_mode="median")
    with pytest.raises(ValueError, match="int16"):
        remove_common_mode(raw, "mean", use_engine=False)
    assert len(predict_recording(m, "MTL", raw, use_engine=False, common_mode="median", decimate=1)["positions"]) == 2


def _infer(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "infer.py"), "--backend", "torch", "--out", str(tmp_path / "o.csv")]
    return subprocess.run(cmd + [str(a) for a in extra], capture_output=True, text=True, cwd=str(tmp_path))


def test_cli_writes_the_map_with_the_common_mode(tmp_path):
    rng = np.random.default_rng(8)
    rec = rng.standard_normal((100, 500)).astype(np.float32) + rng.standard_normal(500).astype(np.float32) * 3
    np.save(tmp_path / "rec.npy", rec)
    np.save(tmp_path / "raw.npy", np.zeros((100, 500), dtype=np.int16))
    r = _infer(tmp_path, "--recording", tmp_path / "rec.npy", "--common_mode", "median", "--map", tmp_path / "m.npz",
               "--batch_size", 4)
    assert r.returncode == 0, r.stderr[-800:]
    z = np.load(tmp_path / "m.npz")
    assert str(z["common_mode"]) == "median" and z["event_map"].shape == (2, 1, 4)
    assert len((tmp_path / "o.csv").read_text().splitlines()) == 4  # header + 3 windows
    os.remove(tmp_path / "o.csv")
    for argv, word in ((["--recording", tmp_path / "rec.npy", "--common_mode", "max"], "--common_mode"),
                       (["--recording", tmp_path / "raw.npy", "--common_mode", "mean"], "int16"),
                       (["--recording", tmp_path / "raw.npy", "--common_mode", "mean", "--chunk", 100], "int16")):
        r = _infer(tmp_path, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.returncode, r.stderr[-400:])
        assert not (tmp_path / "o.csv").exists()
