"""GPU: csrc/common_mode.hip against the definition (data/common_mode.py), bit for bit -- over the shapes, the data
that tries the selection's key (ties, signed zeros, denormals, infinities, NaN of every kind) and the layouts (row
pitch, in place, the surroundings of every output) -- the independence of the time columns, the refusals, and
remove_common_mode / predict_recording(common_mode=...) / LiveRecording(common_mode=...) on the engine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOWS = ("median", "mean")
KINDS = ("randn", "ties", "equal", "zeros", "denormal", "inf", "nan10", "nan60")
FS, NS, CS = (1, 2, 3, 64, 65, 257, 1000, 4099), (1, 31, 32, 33, 200), (1, 2)
PAD = 5
_refs = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _data(kind, rng, shape):
    C, Fn, n = shape
    x = rng.standard_normal(shape).astype(np.float32)
    if kind == "ties":
        x = rng.integers(-2, 3, shape).astype(np.float32)
    elif kind == "equal":  # a column of one value
        x = np.broadcast_to(x[:, :1, :], shape).copy()
    elif kind == "zeros":  # zeros of both signs, and a few columns' worth of other values around them
        x = np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0))
        x = np.where(rng.random(shape) < 0.2, rng.integers(-1, 2, shape).astype(np.float32), x).astype(np.float32)
    elif kind == "denormal":
        x = (rng.integers(-2000, 2001, shape) * 2.0 ** -149).astype(np.float32)
    elif kind == "inf":
        u = rng.random(shape)
        x[u < 0.05], x[u > 0.95] = -np.inf, np.inf
    elif kind in ("nan10", "nan60"):  # quiet, sign-set and signalling NaN
        u = rng.random(shape)
        nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800123], dtype=np.uint32).view(np.float32)
        x = np.where(u < (0.1 if kind == "nan10" else 0.6), nan[rng.integers(0, 4, shape)], x)
    return np.ascontiguousarray(x, dtype=np.float32)


def _shapes():
    from mtl_das_pytorch_amd.ops.hip import lib
    tile = lib().COMMON_MODE_TILE
    shapes = [(C, Fn, n) for C in CS for Fn in FS for n in NS]
    # the kernel has one path; its two block-level seams are the tile of columns and the mean's slab of 256 rows
    shapes += [(2, 5, k * tile + d) for k in (1, 3) for d in (-1, 0, 1)]
    shapes += [(1, Fn, tile + 1) for Fn in (255, 256, 512, 513)]
    return shapes


def _check_launch(HF, x, how):
    """One shape: out of place with a row pitch of n + PAD (NaN beyond n: a finite column stays finite only if it is
    not read), NaN around out and trace; then in place.  Everything equals the definition's bits."""
    from mtl_das_pytorch_amd.data.common_mode import common_mode_reference
    C, Fn, n = x.shape
    want_y, want_m = common_mode_reference(x, how)
    full = np.full((C, Fn, n + PAD), np.nan, dtype=np.float32)
    full[:, :, :n] = x
    x_d = torch.from_numpy(full).cuda()
    out_flat = torch.full((C * Fn * n + 64,), float("nan"), device="cuda")
    tr_flat = torch.full((C * n + 64,), float("nan"), device="cuda")
    out, tr = out_flat[32:32 + C * Fn * n].view(C, Fn, n), tr_flat[32:32 + C * n].view(C, n)
    HF.common_mode(x_d[:, :, :n], how, out=out, trace=tr)
    got, got_m = out_flat.cpu().numpy(), tr_flat.cpu().numpy()
    tag = (how, x.shape)
    y, m = got[32:-32].reshape(C, Fn, n), got_m[32:-32].reshape(C, n)
    for g, w in ((y, want_y), (m, want_m)):
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), tag
        assert np.array_equal(_bits(g)[~nan], _bits(w)[~nan]), tag
    assert np.isnan(got[:32]).all() and np.isnan(got[-32:]).all(), tag
    assert np.isnan(got_m[:32]).all() and np.isnan(got_m[-32:]).all(), tag
    assert np.array_equal(_bits(x_d.cpu().numpy()), _bits(full)), tag  # the input is read only
    # in place, on the pitched rows: the same bits (NaN payloads too: the same instructions), the pad untouched
    x_in = x_d[:, :, :n]
    got_in, _ = HF.common_mode(x_in, how, out=x_in)
    assert got_in.data_ptr() == x_d.data_ptr()
    back = x_d.cpu().numpy()
    assert np.array_equal(_bits(back[:, :, :n]), _bits(y)) and np.isnan(back[:, :, n:]).all(), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", HOWS)
def test_bit_equal_to_the_definition(how, kind):
    from mtl_das_pytorch_amd.ops import functional as HF
    rng = np.random.default_rng(KINDS.index(kind))
    for shape in _shapes():
        _check_launch(HF, _data(kind, rng, shape), how)


@pytest.mark.parametrize("how", HOWS)
def test_every_cut_of_a_stream_gives_the_same_bits(how):
    from mtl_das_pytorch_amd.ops import functional as HF
    x = torch.randn(2, 300, 900, generator=torch.Generator().manual_seed(11)).cuda()
    runs = []
    for cuts in ([900], [1, 47, 48, 49, 3, 752], [1] * 200 + [700]):
        out, tr, at = torch.empty_like(x), torch.empty(2, 900, device="cuda"), 0
        for n in cuts:
            y, m = HF.common_mode(x[:, :, at:at + n], how)  # a slice along time: row pitch 900
            out[:, :, at:at + n], tr[:, at:at + n] = y, m
            at += n
        assert at == 900
        runs.append((out, tr))
    for out, tr in runs[1:]:
        assert torch.equal(out.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(tr.view(torch.int32), runs[0][1].view(torch.int32))


def test_refusals_write_nothing():
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib, ptr, stream
    C, Fn, n = 2, 7, 40
    max_f = lib().COMMON_MODE_MAX_F
    assert max_f >= 65536
    x = torch.randn(C, Fn, n, device="cuda")
    keep = x.clone()
    out = torch.full((C, Fn, n), float("nan"), device="cuda")
    tr = torch.full((C, n), float("nan"), device="cuda")
    ok = {"x": ptr(x), "out": ptr(out), "trace": ptr(tr), "rows": C, "F": Fn, "n": n, "pitch": n, "out_pitch": n,
          "how": 0}
    bad = [dict(ok, how=2), dict(ok, how=-1), dict(ok, x=0), dict(ok, out=0), dict(ok, pitch=n - 1),
           dict(ok, out_pitch=n - 1), dict(ok, F=0), dict(ok, F=max_f + 1), dict(ok, n=1 << 31), dict(ok, n=-1),
           dict(ok, rows=0), dict(ok, rows=1 << 30, F=1),  # 2^30 rows of two tiles: 2^31 blocks
           dict(ok, out=ptr(x) + 4), dict(ok, out=ptr(x), out_pitch=n + 1),  # neither in place nor apart
           dict(ok, trace=ptr(x)), dict(ok, trace=ptr(out) + 4 * (C * Fn * n - 1))]
    for d in bad:
        with pytest.raises(ValueError):
            lib().common_mode(stream(), d)
    lib().common_mode(stream(), dict(ok, n=0, pitch=0, out_pitch=0))  # nothing to do: no launch, no error
    lib().common_mode(stream(), dict(ok, n=0))
    # the wrapper refuses the same before the launch
    wide = torch.zeros(1, max_f + 1, 1, device="cuda")
    for call in (lambda: HF.common_mode(x, "max", out=out, trace=tr),
                 lambda: HF.common_mode(x, None, out=out, trace=tr),
                 lambda: HF.common_mode(x.transpose(1, 2), "median"),
                 lambda: HF.common_mode(x, "median", out=out.transpose(1, 2)),
                 lambda: HF.common_mode(x[0], "median"),
                 lambda: HF.common_mode(x, "median", out=out[:, :, :-1], trace=tr),
                 lambda: HF.common_mode(x, "median", out=out, trace=tr[:, :-1].contiguous()),
                 lambda: HF.common_mode(x, "median", out=out, trace=tr.t()),
                 lambda: HF.common_mode(x[:, :, :-1], "mean", out=x[:, :, 1:]),
                 lambda: HF.common_mode(x, "mean", out=out, trace=out[0, :2]),
                 lambda: HF.common_mode(wide, "median")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: HF.common_mode(x.double(), "median"), lambda: HF.common_mode(x, "median", out=out.double()),
                 lambda: HF.common_mode(x, "median", out=out, trace=tr.double()),
                 lambda: HF.common_mode(x.to(torch.int16), "median")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(RuntimeError):
        HF.common_mode(x.cpu(), "median")
    y, m = HF.common_mode(x[:, :, :0], "median")  # no columns: nothing launched
    assert y.shape == (C, Fn, 0) and m.shape == (C, 0)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(tr).all() and torch.equal(x, keep)


# ---------------------------------------------------------------------------------------------------------------
E2E_F, E2E_STRIDE, E2E_CELL, CHUNKS, RAW_CHUNKS = 200, (100, 125), (50, 125), (1, 249, 130, 77, 443), \
    (1, 747, 390, 231, 1377)
E2E_T = 3 * 899 + 49  # raw samples of 900 decimated ones with the default 49 taps
GATE = dict(gate_db=3.0, noise_floor=1.0)
_cache = {}


def _model(model_type):
    from mtl_das_pytorch_amd.models import build_model
    if model_type not in _cache:
        torch.manual_seed(1)
        m = build_model(model_type)
        m.train()  # non-trivial BN running statistics, so eval mode is exercised
        with torch.no_grad():
            m(torch.randn(8, 1, 100, 250))
        _cache[model_type] = m.eval()
    return _cache[model_type]


def _fixture():
    """(burst-free, recorded): 200 x 900 unit noise, an event (x 6) on fibers 100-199 from t = 500, and on the
    recorded one a common-mode burst 5 randn on every fiber for t in [200, 450)."""
    if "fix" not in _cache:
        g = torch.Generator().manual_seed(3)
        clean = torch.randn(200, 900, generator=g)
        clean[100:, 500:] *= 6.0
        rec = clean.clone()
        rec[:, 200:450] += 5.0 * torch.randn(250, generator=g)
        _cache["fix"] = (clean, rec)
    return _cache["fix"]


def _raw(kind):
    """The 2,746-sample raw streams with a common mode over a third of them."""
    g = torch.Generator().manual_seed(3)
    raw = torch.randn(E2E_F, E2E_T, generator=g)
    raw[100:, 900:2000] *= 6.0
    raw[:, 600:1500] += 5.0 * torch.randn(900, generator=g)
    return (raw * 300).round().to(torch.int16) if kind == "int16" else raw


def _offline(model_type):
    """predict_recording(common_mode="median") of the fixture (Model A: gated too) and of both raw streams
    (decimate=3), on one kept runner."""
    from mtl_das_pytorch_amd.inference import predict_recording, window_runner
    key = ("off", model_type)
    if key not in _cache:
        m = _model(model_type)
        runner = window_runner(m, model_type, 8, torch.device("cuda"))
        kw = dict(stride=E2E_STRIDE, batch=8, device="cuda", use_engine=True, runner=runner, common_mode="median")
        res = {"rec": predict_recording(m, model_type, _fixture()[1], **kw)}
        for kind in ("real", "int16"):
            res[kind] = predict_recording(m, model_type, _raw(kind), decimate=3, **kw)
        if model_type == "MTL":
            res["gated"] = predict_recording(m, model_type, _fixture()[1], **kw, **GATE)
        runner.close()
        _cache[key] = res
    return _cache[key]


def _live(model_type, chunks, sizes, **kw):
    from mtl_das_pytorch_amd.inference import LiveRecording
    live = LiveRecording(_model(model_type), model_type, E2E_F, stride=E2E_STRIDE, cell=E2E_CELL, ring=512, batch=8,
                         device="cuda", use_engine=True, **kw)
    outs, at, caps = [], 0, []
    for i, n in enumerate(sizes):
        chunk = chunks[:, at:at + n]
        if i % 2:  # device and host chunks; the caller's device chunk is not the one that is cleaned
            chunk = chunk.cuda()
            keep = chunk.clone()
        outs.append(live.push(chunk))
        if i % 2:
            assert torch.equal(chunk, keep)
        caps.append(live.captures)
        at += n
    assert at == chunks.shape[1]
    outs.append(live.flush())
    caps.append(live.captures)
    total = live.total
    live.close()
    assert caps == [1] * len(caps), caps
    assert total == 900
    return outs


def _assert_same_windows(outs, off, keys_extra=()):
    pos = np.concatenate([o["positions"] for o in outs])
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    assert len(pos) == 14 and np.array_equal(pos[order], off["positions"])
    keys = [k for k in off if k.endswith("_prob") or k.endswith("_pred")] + list(keys_extra)
    assert [k for k in keys if k.endswith("_prob")]
    for k in keys:
        got = np.concatenate([o[k] for o in outs])[order]
        assert got.dtype == off[k].dtype and np.array_equal(got, off[k]), k


@pytest.mark.parametrize("how", HOWS)
def test_remove_common_mode_on_the_device(how):
    from mtl_das_pytorch_amd.data.common_mode import common_mode_reference
    from mtl_das_pytorch_amd.inference import remove_common_mode
    rec = _fixture()[1]
    want_y, want_m = common_mode_reference(rec.numpy(), how)
    rec_d = rec.cuda()
    for src in (rec, rec_d, rec_d.unsqueeze(0), rec.double()):
        y, m = remove_common_mode(src, how, device="cuda")
        assert y.is_cuda and m.is_cuda and y.shape == (1, 200, 900) and m.shape == (1, 900)
        assert y.data_ptr() != rec_d.data_ptr()
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want_y)), how
        assert np.array_equal(_bits(m.cpu().numpy()), _bits(want_m)), how
    assert torch.equal(rec_d.cpu(), rec)  # the caller's device tensor is as it was


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_live_engine_matches_predict_recording(model_type):
    """LiveRecording(common_mode="median") on host and device chunks: the windows, predictions and probabilities of
    predict_recording(common_mode="median"), bit-equal (every column is cleaned by itself, the rest is the live
    path's existing equality); the stage is outside the graph, which is captured once."""
    off = _offline(model_type)["rec"]
    _assert_same_windows(_live(model_type, _fixture()[1], CHUNKS, common_mode="median"), off)


@pytest.mark.parametrize("kind", ["real", "int16"])
@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_live_decimated_engine_matches_predict_recording(model_type, kind):
    off = _offline(model_type)[kind]
    outs = _live(model_type, _raw(kind), RAW_CHUNKS, decimate=3, common_mode="median")
    _assert_same_windows(outs, off, ("raw_time_start", "raw_time_stop"))


def test_live_gated_matches_offline_and_the_burst_free_flags():
    from mtl_das_pytorch_amd.inference import WINDOW, active_reference, window_power_reference, window_starts
    clean, rec = _fixture()
    fs, ts = window_starts(E2E_F, WINDOW[0], E2E_STRIDE[0]), window_starts(900, WINDOW[1], E2E_STRIDE[1])
    want = active_reference(window_power_reference(clean, fs, ts), len(ts), **GATE)
    off = _offline("MTL")["gated"]
    assert want.sum() == 4 and np.array_equal(off["active"], want)
    outs = _live("MTL", rec, CHUNKS, common_mode="median", **GATE)
    _assert_same_windows(outs, off, ("active",))
    # without the stage the burst opens the gate on the whole fiber
    from mtl_das_pytorch_amd.inference import predict_recording
    plain = predict_recording(_model("MTL"), "MTL", rec, stride=E2E_STRIDE, batch=8, device="cuda", use_engine=True,
                              **GATE)
    assert plain["active"].sum() == 11


@pytest.mark.parametrize("how", HOWS)
def test_predict_recording_is_predict_recording_on_the_cleaned_tensor(how):
    from mtl_das_pytorch_amd.inference import predict_recording, remove_common_mode, window_runner
    m, rec = _model("MTL"), _fixture()[1]
    runner = window_runner(m, "MTL", 8, torch.device("cuda"))
    kw = dict(stride=E2E_STRIDE, batch=8, device="cuda", use_engine=True, runner=runner, **GATE)
    clean = remove_common_mode(rec, how, device="cuda")[0]
    got, want = predict_recording(m, "MTL", rec, common_mode=how, **kw), predict_recording(m, "MTL", clean, **kw)
    runner.close()
    assert set(got) == set(want) and got["active"].sum() == 4
    for k in want:
        assert np.array_equal(got[k], want[k]), k
