"""CPU: raw-rate recordings -- the fp64 definition of the FIR decimation against np.convolve, the default taps'
response, the host's bookkeeping of a decimated stream against brute force, the chunk invariance of the host front
end, the torch backend of LiveRecording(decimate=...) against predict_recording on the decimated recording, and
infer.py's argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

GEOMS = [(1, 1), (1, 5), (2, 5), (3, 7), (4, 1), (5, 2), (4, 4)]  # (D, L)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _K(T, L, D):
    return (T - L) // D + 1 if T >= L else 0


@pytest.mark.parametrize("D,L", GEOMS)
def test_reference_is_the_valid_convolution_subsampled(D, L):
    from mtl_das_pytorch_amd.data.resample import fir_decimate_reference, output_count
    rng = np.random.default_rng(10 * D + L)
    h = rng.standard_normal(L)
    for T in range(max(L - 1, 0), L + 3 * D + 2):
        x = rng.standard_normal((2, 3, T))
        got = fir_decimate_reference(x, h, D)
        assert got.dtype == np.float64 and got.shape == (2, 3, _K(T, L, D)) and output_count(T, L, D) == _K(T, L, D)
        if T < L:
            continue
        want = np.stack([[np.convolve(r, h, "valid")[::D] for r in c] for c in x])
        assert np.abs(got - want).max() <= 1e-12, (T, np.abs(got - want).max())
    # the special cases: plain subsampling and the block mean
    x = rng.standard_normal(40)
    assert np.array_equal(fir_decimate_reference(x, [1.0], 4), x[::4])
    assert np.abs(fir_decimate_reference(x, np.ones(4) / 4, 4) - x.reshape(10, 4).mean(1)).max() <= 1e-15


def _response_db(h):
    """(f, dB) of the taps' magnitude response on the 20,001-point grid over [0, 0.5] cycles per raw sample."""
    f = np.linspace(0.0, 0.5, 20001)
    H = np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(len(h))[None]) @ h)
    with np.errstate(divide="ignore"):
        return f, 20 * np.log10(H)


@pytest.mark.parametrize("D", [2, 3, 4, 5, 8, 10, 16])
def test_default_taps(D):
    from mtl_das_pytorch_amd.data.resample import decimation_taps
    h = decimation_taps(D)
    assert h.dtype == np.float64 and len(h) == 16 * D + 1
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - 1) <= 1e-15
    f, db = _response_db(h)
    stop = db[f >= 0.5 / D].max()
    print(f"D = {D}: stop band {stop:.2f} dB")
    assert stop <= -50.0, stop
    band = np.abs(db[f <= 0.25 / D]).max()
    print(f"D = {D}: pass band deviation {band:.5f} dB")
    assert band <= 0.01, band


def test_default_taps_of_one_and_limits():
    from mtl_das_pytorch_amd.data.resample import DecimatorBook, as_taps, decimation_taps
    assert np.array_equal(decimation_taps(1), [1.0])
    assert as_taps(None, 4).dtype == np.float32 and len(as_taps(None, 4)) == 65
    for D, L in [(0, 1), (65, 1), (1, 1026), (1, 0)]:
        with pytest.raises(ValueError):
            DecimatorBook(L, D)
        with pytest.raises(ValueError):
            as_taps(np.ones(L), D)
    with pytest.raises(ValueError):
        as_taps(np.ones((2, 2)), 2)


@pytest.mark.parametrize("D,L", GEOMS)
def test_book_matches_brute_force(D, L):
    from mtl_das_pytorch_amd.data.resample import DecimatorBook
    sizes = [1, L - 1, L, D, D + 1, 50]
    for chunks in (sizes, sizes[::-1], [1] * 9 + sizes, [50, 1, 1, D + 1, L, 1]):
        chunks = [n for n in chunks if n > 0]
        book = DecimatorBook(L, D)
        total, seen = 0, []
        for n in chunks:
            before = (book.carry_len, book.skip)
            assert book.plan([n, 3]) == book.plan([n, 3]) and (book.carry_len, book.skip) == before  # a dry run
            m, carry_len, skip = book.push(n)
            assert (carry_len, skip) == before
            seen += list(range(book.k_next - m, book.k_next))
            total += n
            assert book.raw_total == total and book.k_next == _K(total, L, D)
            assert book.carry_len == max(0, total - book.k_next * D) <= L - 1
            assert book.skip == max(0, book.k_next * D - total)
            assert book.skip == 0 or D > L
            # the count the launch is checked against: the piece's stream is the carry and the raw samples after skip
            ns = carry_len + max(0, n - skip)
            assert m == _K(ns, L, D)
        assert seen == list(range(_K(total, L, D)))  # each output once, in order


@pytest.mark.parametrize("D,L", GEOMS + [(3, 49)])
def test_host_front_end_is_chunk_invariant(D, L):
    """Piecewise with the carry, as the torch backend of LiveRecording runs it: equal to the one-shot reference."""
    from mtl_das_pytorch_amd.data.resample import HostDecimator, fir_decimate_reference
    rng = np.random.default_rng(L)
    h = rng.standard_normal(L).astype(np.float32)
    x = rng.standard_normal((2, 3, 311)).astype(np.float32)
    want = fir_decimate_reference(x, h, D)
    for chunks in ([311], [1, 47, 48, 49, 3, 100, 63], [1] * 60 + [251], [L, D, D + 1, 311 - L - 2 * D - 1]):
        assert sum(chunks) == 311
        dec, got, at = HostDecimator(h, D), [], 0
        for n in chunks:
            got.append(dec.push(x[..., at:at + n]))
            at += n
        got = np.concatenate(got, -1)
        assert got.shape == want.shape and (got == want).all(), chunks
        assert dec.carry.shape[-1] == dec.book.carry_len <= L - 1


# ---------------------------------------------------------------------------------------------------------------
F_, D_, STRIDE, CELL, RAW_CHUNKS = 200, 3, (100, 125), (50, 125), (1, 747, 390, 231, 1377)
T_RAW = 3 * 899 + 49  # K = 900 with the default 49 taps
_cache = {}


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


def _runs():
    from mtl_das_pytorch_amd.data.resample import decimation_taps
    from mtl_das_pytorch_amd.inference import LiveRecording, decimate_recording, predict_recording
    if "runs" not in _cache:
        raw = torch.randn(F_, T_RAW, generator=torch.Generator().manual_seed(5))
        taps = decimation_taps(D_)
        rec = decimate_recording(raw, D_, taps, use_engine=False)
        assert rec.shape == (1, F_, 900) and rec.dtype == torch.float32
        off = predict_recording(_model(), "MTL", rec, stride=STRIDE, batch=8, use_engine=False)
        off_raw = predict_recording(_model(), "MTL", raw, stride=STRIDE, batch=8, use_engine=False, decimate=D_)
        live = LiveRecording(_model(), "MTL", F_, stride=STRIDE, cell=CELL, ring=512, batch=8, use_engine=False,
                             decimate=D_, taps=taps)
        outs, at = [], 0
        for n in RAW_CHUNKS:
            outs.append(live.push(raw[:, at:at + n]))
            at += n
        assert at == T_RAW and live.total == 900 and live.dbook.raw_total == T_RAW
        outs.append(live.flush())
        live.close()
        _cache["runs"] = (rec, off, off_raw, outs)
    return _cache["runs"]


def test_torch_live_decimated_matches_predict_recording():
    rec, off, off_raw, outs = _runs()
    pos = np.concatenate([o["positions"] for o in outs])
    assert len(pos) == len(off["positions"]) == 14
    assert len(outs[0]["positions"]) == 0 and outs[0]["distance_prob"].shape == (0, 16)  # one raw sample: no output
    assert outs[0]["map_columns"]["event_map"].shape == (2, 4, 0)
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    order_off = np.lexsort((off["positions"][:, 1], off["positions"][:, 0]))
    assert np.array_equal(pos[order], off["positions"][order_off])
    for k in ("distance_pred", "event_pred"):
        assert np.array_equal(np.concatenate([o[k] for o in outs])[order], off[k][order_off])
    for k in ("distance_prob", "event_prob"):
        got = np.concatenate([o[k] for o in outs])[order]
        err = np.abs(got.astype(np.float64) - off[k][order_off]).max()
        print(f"torch live (decimated) vs offline {k}: max abs diff {err:.3e}")
        assert err <= 1e-5, (k, err)
    # raw extents: 49 taps, windows of 250 decimated samples
    for res in [off_raw] + outs:
        t0 = res["positions"][:, 1]
        assert np.array_equal(res["raw_time_start"], t0 * 3)
        assert np.array_equal(res["raw_time_stop"], (t0 + 249) * 3 + 49)
    assert off_raw["raw_time_stop"].max() == T_RAW
    assert "raw_time_start" not in off
    # predict_recording(decimate=) is predict_recording on decimate_recording
    for k in off:
        assert np.array_equal(off[k], off_raw[k]), k


def test_torch_live_decimated_map_columns_match_prediction_map():
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map, window_starts
    rec, off, _, outs = _runs()
    fs, ts = window_starts(F_, WINDOW[0], STRIDE[0]), window_starts(900, WINDOW[1], STRIDE[1])
    want = prediction_map(off, fs, ts, (F_, 900), CELL)
    at = 0
    for o in outs:  # each column once, in order
        mc = o["map_columns"]
        assert mc["first"] == at and mc["last"] >= at
        at = mc["last"]
    assert at == want["event_map"].shape[2] == 8
    for k in ("event_map", "distance_map", "distance_mean_m"):
        got = np.concatenate([o["map_columns"][k] for o in outs], -1)
        err = np.abs(got - want[k]).max()
        print(f"torch live (decimated) map {k}: max abs diff {err:.3e}")
        assert got.shape == want[k].shape and err <= 1e-6, (k, err)


def test_int16_and_refusals():
    from mtl_das_pytorch_amd.inference import LiveRecording, decimate_recording, predict_recording
    from mtl_das_pytorch_amd.data.resample import fir_decimate_reference
    raw = torch.randint(-300, 300, (1, 4, 90), generator=torch.Generator().manual_seed(1)).to(torch.int16)
    got = decimate_recording(raw, 4, [0.5, 0.25, 0.25], use_engine=False)
    assert np.array_equal(got.numpy(), fir_decimate_reference(raw.numpy(), [0.5, 0.25, 0.25], 4).astype(np.float32))
    m = _model()
    with pytest.raises(ValueError):
        predict_recording(m, "MTL", torch.zeros(100, 300), use_engine=False, taps=[1.0])  # taps without decimate
    for kw in (dict(decimate=0), dict(decimate=65), dict(decimate=2, taps=np.ones(1026)), dict(taps=[1.0])):
        with pytest.raises(ValueError):
            LiveRecording(m, "MTL", 100, use_engine=False, **kw)
    # the table check runs before anything is written: 3 time indices do not hold this push
    live = LiveRecording(m, "MTL", 100, stride=(100, 10), ring=512, use_engine=False, table_indices=3, decimate=2,
                         taps=[0.5, 0.5])
    with pytest.raises(ValueError):
        live.push(torch.zeros(100, 2 * 400))
    assert live.total == 0 and live.dbook.raw_total == 0 and torch.isnan(live.backend.ring).all()
    live.flush()
    with pytest.raises(RuntimeError):
        live.push(torch.zeros(100, 1))


def _infer(tmp_path, *extra):
    np.save(tmp_path / "rec.npy", np.zeros((100, 600), dtype=np.float32))
    np.save(tmp_path / "raw.npy", np.zeros((100, 600), dtype=np.int16))
    cmd = [sys.executable, os.path.join(ROOT, "infer.py"), "--backend", "torch", "--out", str(tmp_path / "o.csv")]
    return subprocess.run(cmd + [str(a) for a in extra], capture_output=True, text=True, cwd=str(tmp_path))


def test_cli_argument_errors(tmp_path):
    np.save(tmp_path / "long.npy", np.ones(1026))
    np.save(tmp_path / "taps.npy", np.ones(4) / 4)
    rec, raw = tmp_path / "rec.npy", tmp_path / "raw.npy"
    bad = [
        (["--recording", rec, "--taps", tmp_path / "taps.npy"], "--taps needs --decimate"),
        (["--recording", rec, "--decimate", 0], "--decimate"),
        (["--recording", rec, "--decimate", 65], "--decimate"),
        (["--recording", rec, "--decimate", 2, "--taps", tmp_path / "long.npy"], "1025"),
        (["--recording", raw], "int16"),
        (["--recording", raw, "--chunk", 100], "int16"),
    ]
    for argv, word in bad:
        r = _infer(tmp_path, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.returncode, r.stderr[-400:])
        assert not (tmp_path / "o.csv").exists()
