"""CPU: the activity gate of a growing recording -- the causal running noise floor against a plain-Python loop, the
fixture's flags in fp64 (and the two conditions that make them a fair test), the torch backend of
LiveRecording(gate_db=...) against the references, predict_recording and prediction_map, LiveBook's history, and the
command line.

Fixture: gate_ref's recording cut to T = 690 at stride (10, 50) and 3 dB: fiber starts 0 .. 130 (14), time starts
0 .. 400 and the end-aligned 440 (10) -- 140 windows, live number n = j * 14 + a."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_ = 690
CHUNKS = (1, 249, 130, 77, 233)
HISTORY, WARMUP = 4, 2
_cache = {}


def fixture():
    """(rec [230, 690] fp32, fs, ts, power fp64 [10 * 14] in live numbering)."""
    if "fix" not in _cache:
        from mtl_das_pytorch_amd.inference import WINDOW, window_power_reference, window_starts
        rec = G.fixture()[0][:, :T_].copy()
        fs, ts = window_starts(230, WINDOW[0], G.STRIDE[0]), window_starts(T_, WINDOW[1], G.STRIDE[1])
        assert len(fs) == 14 and list(ts) == list(range(0, 401, 50)) + [440] and sum(CHUNKS) == T_
        power = window_power_reference(rec, fs, ts, WINDOW).reshape(14, 10).T.reshape(-1).copy()
        _cache["fix"] = (rec, fs, ts, power)
    return _cache["fix"]


def fixture_flags(noise_floor):
    """(active [10, 14] bool, floor [10, 14]) of the fixture by the fp64 references, after gate_ref.fixture_flags' two
    conditions: no window within 0.01 dB of its threshold and an active share of 20 % .. 80 %."""
    from mtl_das_pytorch_amd.inference import live_active_reference, running_floor_reference
    power = fixture()[3].reshape(10, 14)
    if noise_floor == "running":
        floor = running_floor_reference(power.reshape(-1), 14, HISTORY, WARMUP)
    else:
        floor = np.full(power.shape, float(noise_floor))
    active = live_active_reference(power, floor, G.GATE_DB)
    thr = floor * 10.0 ** (G.GATE_DB / 10.0)
    with np.errstate(divide="ignore"):
        margin = np.abs(10.0 * np.log10(power / thr))  # inf where there is no floor yet
    print(f"noise_floor={noise_floor}: {int(active.sum())} of {active.size} active, nearest {margin.min():.3f} dB")
    assert margin.min() > 0.01, margin.min()
    assert 0.2 <= active.mean() <= 0.8, active.mean()
    return active, floor


@pytest.mark.parametrize("history", [1, 3, 4])
@pytest.mark.parametrize("warmup", [1, 2])
def test_running_floor_reference_matches_a_plain_loop(history, warmup):
    from mtl_das_pytorch_amd.inference import live_active_reference, running_floor_reference
    if warmup > history:
        with pytest.raises(ValueError):
            running_floor_reference(np.zeros(6), 3, history, warmup)
        return
    nj, nf = 9, 3
    p = np.random.default_rng(5).random((nj, nf))
    p[4, 1] = np.nan       # ordered last, as np.sort does
    p[2, 0] = p[3, 0]      # tied values
    p[6, 2] = p[5, 2] = p[4, 2]
    got = running_floor_reference(p.reshape(-1), nf, history, warmup)
    assert got.shape == (nj, nf)
    nan_floor = 0
    for j in range(nj):
        for a in range(nf):
            v = [p[i, a] for i in range(max(0, j - history + 1), j + 1)]
            m = len(v)
            want = sorted(v, key=lambda x: (x != x, x))[(m - 1) // 2] if m >= warmup else 0.0
            if m < warmup:
                assert got[j, a] == 0.0  # exactly: "no floor yet"
            assert got[j, a] == want or (want != want and got[j, a] != got[j, a]), (j, a)
            nan_floor += int(want != want)
    assert (nan_floor > 0) == (history == 1)  # a NaN is the median only of itself
    # a floor of 0 and a NaN power are active, whatever the gate
    act = live_active_reference(p, got, 60.0)
    assert act[4, 1] and act[got == 0].all() and not act[(got > 0) & ~np.isnan(p)].any()


def test_fixture_flags_are_what_the_fixture_was_chosen_for():
    active, floor = fixture_flags("running")
    assert active.sum() == 46 and active.sum(1).tolist() == [14, 0, 0, 0, 0, 10, 12, 10, 0, 0]
    assert (floor[0] == 0).all() and (floor[1:] > 0).all()  # warmup = 2: no floor at the first index only
    active, _ = fixture_flags(1.0)
    assert active.sum() == 60


def _model_a():
    """Model A with the count of windows its forward has seen."""
    if "m" not in _cache:
        from mtl_das_pytorch_amd.models import build_model
        torch.manual_seed(0)
        m = build_model("MTL").eval()
        seen = [0]
        forward = m.forward

        def counted(x):
            seen[0] += len(x)
            return forward(x)

        m.forward = counted
        _cache["m"] = (m, seen)
    return _cache["m"]


def _live(noise_floor, cell=None):
    """The gated torch-backend run of the fixture in CHUNKS: (outs, rows the module saw)."""
    key = ("live", noise_floor, cell)
    if key not in _cache:
        from mtl_das_pytorch_amd.inference import LiveRecording
        m, seen = _model_a()
        rec = torch.from_numpy(fixture()[0])
        seen[0] = 0
        live = LiveRecording(m, "MTL", 230, stride=G.STRIDE, cell=cell, ring=512, batch=35, use_engine=False,
                             gate_db=G.GATE_DB, noise_floor=noise_floor, floor_history=HISTORY, floor_warmup=WARMUP)
        outs, at = [], 0
        for n in CHUNKS:
            outs.append(live.push(rec[:, at:at + n]))
            at += n
        outs.append(live.flush())
        live.close()
        _cache[key] = (outs, seen[0])
    return _cache[key]


def _cat(outs, k):
    return np.concatenate([o[k] for o in outs])


@pytest.mark.parametrize("noise_floor", ["running", 1.0])
def test_torch_live_gate_matches_the_reference(noise_floor):
    want, floor = fixture_flags(noise_floor)
    outs, seen = _live(noise_floor)
    active = _cat(outs, "active")
    assert active.dtype == bool and np.array_equal(active, want.reshape(-1))  # evaluation order is the live numbering
    assert seen == want.sum()  # the module never saw a quiet window
    power = fixture()[3]
    assert np.allclose(_cat(outs, "power_db"), 10 * np.log10(power), rtol=0, atol=1e-9)
    fdb = _cat(outs, "floor_db")
    with np.errstate(divide="ignore"):
        assert np.array_equal(np.isneginf(fdb), floor.reshape(-1) == 0)
        assert np.allclose(fdb[floor.reshape(-1) > 0], 10 * np.log10(floor.reshape(-1)[floor.reshape(-1) > 0]),
                           rtol=0, atol=1e-9)
    assert np.isneginf(fdb).sum() == (14 if noise_floor == "running" else 0)
    for k in ("distance", "event"):
        pred, prob = _cat(outs, f"{k}_pred"), _cat(outs, f"{k}_prob")
        assert (pred[~active] == -1).all() and (prob[~active] == 0).all()
        assert (pred[active] >= 0).all() and np.allclose(prob[active].sum(1), 1, atol=1e-5)


def test_torch_live_fixed_floor_matches_predict_recording_and_its_map():
    from mtl_das_pytorch_amd.inference import predict_recording, prediction_map
    rec, fs, ts, _ = fixture()
    m, _ = _model_a()
    cell = (50, 50)
    off = predict_recording(m, "MTL", torch.from_numpy(rec), stride=G.STRIDE, batch=35, use_engine=False,
                            gate_db=G.GATE_DB, noise_floor=1.0)
    outs, _ = _live(1.0, cell)
    pos = _cat(outs, "positions")
    order = np.lexsort((pos[:, 1], pos[:, 0]))  # fiber-major, as the offline table
    assert np.array_equal(pos[order], off["positions"])
    assert set(off) | {"floor_db", "map_columns"} == set(outs[-1])
    assert np.array_equal(_cat(outs, "active")[order], off["active"])
    assert np.allclose(_cat(outs, "power_db")[order], off["power_db"], rtol=0, atol=1e-9)
    for k in ("distance", "event"):
        assert np.array_equal(_cat(outs, f"{k}_pred")[order], off[f"{k}_pred"])
        err = np.abs(_cat(outs, f"{k}_prob")[order].astype(np.float64) - off[f"{k}_prob"]).max()
        print(f"gated torch live vs offline {k}_prob: max abs diff {err:.3e}")
        assert err <= 1e-5, (k, err)  # test_live_ref's bound of the ungated run: other batches of the same module
    # the map: columns once and in order; NaN exactly where prediction_map has it; values by test_live_ref's criterion
    want = prediction_map(off, fs, ts, (230, T_), cell)
    at = 0
    for o in outs:
        mc = o["map_columns"]
        assert mc["first"] == at and mc["activity_map"].shape == (5, mc["last"] - at)
        at = mc["last"]
    assert at == want["activity_map"].shape[1] == 14
    for k in ("event_map", "distance_map", "distance_mean_m", "activity_map"):
        got = np.concatenate([o["map_columns"][k] for o in outs], -1)
        assert got.shape == want[k].shape and np.array_equal(np.isnan(got), np.isnan(want[k])), k
        ok = ~np.isnan(got)
        err = np.abs(got[ok] - want[k][ok]).max()
        print(f"gated torch live map {k}: max abs diff {err:.3e}")
        assert err <= 1e-6, (k, err)
    cm = np.concatenate([o["map_columns"]["class_map"] for o in outs], -1)
    assert np.array_equal(cm[:16], np.concatenate([o["map_columns"]["distance_map"] for o in outs], -1),
                          equal_nan=True)  # class_map is the divided map
    # the activity: in [0, 1], and 0 exactly where every covering window is quiet
    act = np.concatenate([o["map_columns"]["activity_map"] for o in outs], -1)
    flags = off["active"].reshape(14, 10)
    covered = np.zeros(act.shape, dtype=bool)
    for i in range(act.shape[0]):
        for q in range(act.shape[1]):
            fa = [a for a, f0 in enumerate(fs) if f0 < min((i + 1) * cell[0], 230) and f0 + 100 > i * cell[0]]
            tb = [b for b, t0 in enumerate(ts) if t0 < min((q + 1) * cell[1], T_) and t0 + 250 > q * cell[1]]
            covered[i, q] = flags[np.ix_(fa, tb)].any()
    assert (act >= 0).all() and (act <= 1 + 1e-12).all() and np.array_equal(act > 0, covered)
    assert (~covered).any() and covered.any()
    assert np.isnan(cm[:, ~covered]).all() and not np.isnan(cm[:, covered]).any()


def test_argument_errors():
    from mtl_das_pytorch_amd.inference import LiveRecording
    m, _ = _model_a()
    kw = dict(stride=G.STRIDE, ring=512, use_engine=False, gate_db=3.0)
    with pytest.raises(ValueError, match="running"):
        LiveRecording(m, "MTL", 230, noise_floor="auto", **kw)
    with pytest.raises(ValueError, match="floor_warmup"):
        LiveRecording(m, "MTL", 230, floor_history=4, floor_warmup=5, **kw)
    with pytest.raises(ValueError, match="1024"):
        LiveRecording(m, "MTL", 230, floor_history=1025, **kw)
    with pytest.raises(ValueError):
        LiveRecording(m, "MTL", 230, floor_history=0, floor_warmup=0, **kw)
    # without a gate nothing about the floor is looked at, and the result has no gate keys
    live = LiveRecording(m, "MTL", 230, noise_floor="auto", stride=G.STRIDE, ring=512, use_engine=False)
    assert "active" not in live.push(torch.zeros(230, 10)) and live.book.history is None


def test_live_book_keeps_the_floor_history():
    from mtl_das_pytorch_amd.inference import LiveBook
    # Wt 7, stride 3, ring 16: a piece adds at most 4 indices; a history of 4 carries 3 more
    assert LiveBook(7, 3, 16).jcap == 4 and LiveBook(7, 3, 16, history=1).jcap == 4
    assert LiveBook(7, 3, 16, history=4).jcap == 7
    assert LiveBook(7, 3, 16, ct=2, history=4).jcap == LiveBook(7, 3, 16, ct=2).jcap  # the columns carry 5 already
    book = LiveBook(7, 3, 16, table_indices=4, history=4)
    book.advance(7)  # one index: 1 + 3 rows of history
    assert (book.total, book.j_done) == (7, 1)
    with pytest.raises(ValueError, match="history"):
        book.check_push(6)  # two indices: the second would overwrite a power row the floor still reads
    with pytest.raises(ValueError, match="history"):
        book.advance(6)
    assert (book.total, book.j_done, book.q_done) == (7, 1, 0)  # nothing changed
    book.advance(3)
    assert book.j_done == 2
    with pytest.raises(ValueError):
        LiveBook(7, 3, 16, history=0)


def _infer(tmp_path, *extra, out="p.csv"):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--model", "MTL", "--recording",
                           str(tmp_path / "rec.npy"), "--out", str(tmp_path / out), *extra], env=env,
                          capture_output=True, text=True, timeout=600)


def test_infer_cli_live_gate(tmp_path):
    import pandas as pd
    rec = np.random.default_rng(0).standard_normal((100, 600)).astype(np.float32)  # test_gate.py's recording
    rec[:, 350:] *= 4
    np.save(tmp_path / "rec.npy", rec)
    r = _infer(tmp_path, "--gate_db", "6", "--noise_floor", "running")
    assert r.returncode == 2 and "--chunk" in r.stderr and not (tmp_path / "p.csv").exists()
    r = _infer(tmp_path, "--gate_db", "6", "--chunk", "200")  # the default floor, "auto", has no stream form
    assert r.returncode == 2 and "--chunk" in r.stderr and "running" in r.stderr and not (tmp_path / "p.csv").exists()
    common = ("--gate_db", "6", "--noise_floor", "1.0", "--stride", "100,100")
    r = _infer(tmp_path, *common, "--chunk", "200", "--map", str(tmp_path / "m.npz"))
    assert r.returncode == 0, r.stderr[-2000:]
    r = _infer(tmp_path, *common, "--map", str(tmp_path / "m0.npz"), out="p0.csv")
    assert r.returncode == 0, r.stderr[-2000:]
    df, df0 = pd.read_csv(tmp_path / "p.csv"), pd.read_csv(tmp_path / "p0.csv")
    assert df["active"].tolist() == [0, 0, 1, 1, 1] and list(df.columns) == list(df0.columns)
    assert {"power_db", "active", "distance_pred", "event_pred"} <= set(df.columns)
    for k in df.columns:
        if k == "power_db":
            assert np.allclose(df[k], df0[k], rtol=0, atol=1e-9)
        elif k.endswith("_pred"):  # the two processes draw their own weights: which windows have a prediction
            assert (df[k] == -1).tolist() == (df0[k] == -1).tolist() == [True, True, False, False, False], k
        else:
            assert df[k].tolist() == df0[k].tolist(), k
    maps, maps0 = np.load(tmp_path / "m.npz"), np.load(tmp_path / "m0.npz")
    assert set(maps.files) == set(maps0.files) and "activity_map" in maps.files
    assert np.allclose(maps["activity_map"], maps0["activity_map"], rtol=0, atol=1e-12)
    for k in ("event_map", "distance_map"):
        assert np.array_equal(np.isnan(maps[k]), np.isnan(maps0[k])), k
        assert np.isnan(maps[k][:, 0, 0]).all() and not np.isnan(maps[k][:, 0, 5]).any()
    # the running floor through the command line: the first index has no floor yet, so it is active
    r = _infer(tmp_path, "--gate_db", "6", "--noise_floor", "running", "--floor_history", "3", "--floor_warmup", "2",
               "--stride", "100,100", "--chunk", "200", out="p2.csv")
    assert r.returncode == 0, r.stderr[-2000:]
    assert pd.read_csv(tmp_path / "p2.csv")["active"].tolist()[0] == 1
