"""GPU: csrc/resample.hip fir_decimate against the fp64 definition (data/resample.py) -- exactly on integer data over
the geometries, carries, skips and tile counts, within the derived fp32 bound on real data, bit-equal for every
chunking -- its refusals, and LiveRecording(decimate=...) on the engine against predict_recording(decimate=...)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMS = [(1, 1), (1, 5), (2, 5), (2, 33), (3, 7), (4, 1), (5, 2), (32, 33), (64, 1)]  # (D, L)
I16_SENTINEL = 32767


def _K(T, L, D):
    return (T - L) // D + 1 if T >= L else 0


def _piece_length(m, carry_len, skip, L, D, extra):
    """Raw samples n of a piece that completes exactly ``m`` outputs after ``carry_len`` / ``skip``."""
    if m == 0:
        ns = max(carry_len, L - 1)  # as long as it can be without an output
    else:
        ns = (m - 1) * D + L + min(extra, D - 1)
    return ns - carry_len + skip


def _launch_and_check(HF, D, L, rows, m, carry_len, skip, dtype, rng, extra):
    from mtl_das_pytorch_amd.data.resample import fir_decimate_reference
    n = _piece_length(m, carry_len, skip, L, D, extra)
    if n < skip:  # (only m = 0, nothing carried) the whole piece is skipped
        n = max(0, skip - 1)
    h = rng.integers(-2, 3, L).astype(np.float32)
    pad = 5
    x = rng.integers(-8, 9, (1, rows, n + pad))
    if dtype == torch.int16:
        x[..., n:] = I16_SENTINEL
        raw_full = torch.from_numpy(x.astype(np.int16)).cuda()
    else:
        raw_full = torch.from_numpy(x.astype(np.float32)).cuda()
        raw_full[..., n:] = float("nan")
    raw = raw_full[..., :n]  # row pitch n + pad
    cin = rng.integers(-8, 9, (rows, L - 1)).astype(np.float32)
    cin_d = torch.from_numpy(cin).cuda()
    cin_d[:, carry_len:] = float("nan")
    out_flat = torch.full((rows * m + 64,), float("nan"), device="cuda")
    cout_flat = torch.full((rows * (L - 1) + 64,), float("nan"), device="cuda")
    out = out_flat[:rows * m].view(1, rows, m)
    cout = cout_flat[:rows * (L - 1)].view(rows, L - 1)
    HF.fir_decimate(raw, cin_d, carry_len, skip, torch.from_numpy(h).cuda(), D, out=out, m=m, carry_out=cout)
    s = np.concatenate([cin[:, :carry_len].astype(np.float64), x[0, :, skip:n].astype(np.float64)], 1)
    want = fir_decimate_reference(s, h, D)
    assert want.shape == (rows, m)
    tag = (D, L, rows, m, carry_len, skip, str(dtype))
    got = out_flat.cpu().numpy()
    assert (got[:rows * m].reshape(rows, m).astype(np.float64) == want).all(), tag
    assert np.isnan(got[rows * m:]).all(), tag
    tail = s[:, m * D:]
    assert tail.shape[1] <= L - 1
    got_c = cout_flat.cpu().numpy()
    body = got_c[:rows * (L - 1)].reshape(rows, L - 1)
    assert (body[:, :tail.shape[1]].astype(np.float64) == tail).all(), tag
    assert np.isnan(body[:, tail.shape[1]:]).all() and np.isnan(got_c[rows * (L - 1):]).all(), tag
    return tail.shape[1]


@pytest.mark.parametrize("D,L", GEOMS)
def test_integer_data_is_exact(D, L):
    """Integers in [-8, 8] times integer taps in [-2, 2], L <= 33: every partial sum is an integer below 2^24, so out
    and carry_out equal the fp64 definition exactly.  NaN (int16: 32767) fills what must not be read -- the raw row
    beyond n, carry_in beyond carry_len -- and what must not be written: out's and carry_out's surroundings."""
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib
    tile = lib().DECIMATE_TILE
    assert tile == HF.DECIMATE_TILE
    rng = np.random.default_rng(100 * D + L)
    states = [(c, 0) for c in sorted({0, min(1, L - 1), L - 1})]
    if D > L:
        states += [(0, 1), (0, D - L)]
    tails, launches = set(), 0
    for rows in (1, 3, 7):
        for m in (0, 1, tile, 2 * tile + 1):
            for carry_len, skip in states:
                for dtype in (torch.float32, torch.int16):
                    tails.add(_launch_and_check(HF, D, L, rows, m, carry_len, skip, dtype, rng, extra=launches % 3))
                    launches += 1
    torch.cuda.synchronize()
    assert max(tails) == L - 1 and (len(tails) > 1 or D == 1 or L == 1)  # full and (D > 1) partial new tails


CASES = [(2, None), (3, None), (10, None), (4, 1025)]  # (D, L): None = the default taps


@pytest.mark.parametrize("D,L", CASES)
def test_real_data_within_the_fp32_bound(D, L):
    """|got - ref| <= (L + 1) 2^-24 sum_i |h_i x_i| per element: L products and L - 1 additions, each rounded once in
    fp32, in any order (an fma rounds less).  The reference gets the taps' fp32 values."""
    from mtl_das_pytorch_amd.data.resample import as_taps, fir_decimate_reference
    from mtl_das_pytorch_amd.ops import functional as HF
    g = torch.Generator().manual_seed(D)
    h = as_taps(None if L is None else torch.randn(L, generator=g).numpy(), D)
    L = len(h)
    n = (2 * HF.DECIMATE_TILE + 40) * D + L  # three tiles, the last one partial
    x = torch.randn(1, 3, n, generator=g)
    got = HF.fir_decimate(x.cuda(), None, 0, 0, torch.from_numpy(h).cuda(), D)[0].cpu().numpy().astype(np.float64)
    ref = fir_decimate_reference(x.numpy(), h, D)
    bound = (L + 1) * 2.0 ** -24 * fir_decimate_reference(x.abs().numpy(), np.abs(h), D)
    assert got.shape == ref.shape == (1, 3, _K(n, L, D))
    err = np.abs(got - ref)
    print(f"fir_decimate D = {D}, L = {L}: worst |err| {err.max():.3e}, worst err / bound {(err / bound).max():.4f}")
    assert (err <= bound).all(), (err / bound).max()


def _stream(HF, x_d, taps_d, D, pieces):
    """The stream ``x_d`` decimated in ``pieces``, the carry buffers flipped as LiveRecording's backend does."""
    from mtl_das_pytorch_amd.data.resample import DecimatorBook
    C, Fn, T = x_d.shape
    book = DecimatorBook(taps_d.numel(), D)
    carry, cur, outs, at = HF.decimate_carry(C * Fn, taps_d.numel(), x_d.device), 0, [], 0
    for n in pieces:
        m, carry_len, skip = book.push(n)
        out, _ = HF.fir_decimate(x_d[:, :, at:at + n], carry[cur], carry_len, skip, taps_d, D, m=m,
                                 carry_out=carry[1 - cur])
        cur, at = 1 - cur, at + n
        outs.append(out)
    assert at == T
    return torch.cat(outs, 2)


def test_every_chunking_gives_the_same_bits():
    from mtl_das_pytorch_amd.data.resample import as_taps
    from mtl_das_pytorch_amd.ops import functional as HF
    T = 3 * 899 + 49
    x = torch.randn(2, 3, T, generator=torch.Generator().manual_seed(7)).cuda()
    taps = torch.from_numpy(as_taps(None, 3)).cuda()
    cuts = [[T], [1, 47, 48, 49, 3, 1000, 1598], [1] * 200 + [T - 200]]
    runs = [_stream(HF, x, taps, 3, c) for c in cuts] + [_stream(HF, x, taps, 3, cuts[1])]
    assert runs[0].shape == (2, 3, 900)
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int32), runs[0].view(torch.int32))
    # subsampling with D > L: the skip across pieces
    one = torch.ones(1, device="cuda")
    for c in ([T], [1, 2, 3, 5, 64, 65, T - 140], [7] * 10 + [T - 70]):
        assert torch.equal(_stream(HF, x, one, 64, c), x[:, :, ::64])


def test_refusals_write_nothing():
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib, ptr, stream
    L, D, n, rows = 5, 2, 40, 3
    raw = torch.randn(1, rows, n, device="cuda")
    taps = torch.ones(L, device="cuda")
    out = torch.full((1, rows, 18), float("nan"), device="cuda")
    cin, cout = (torch.full((rows, L - 1), float("nan"), device="cuda") for _ in range(2))
    ok = {"raw": ptr(raw), "carry_in": ptr(cin), "taps": ptr(taps), "out": ptr(out), "carry_out": ptr(cout),
          "rows": rows, "n": n, "pitch": n, "m": 18, "carry_len": 0, "skip": 0, "D": D, "L": L, "itype": 0}
    assert lib().fir_output_count(0, 0, n, L, D) == 18
    bad = [dict(ok, D=0), dict(ok, D=65), dict(ok, L=1026), dict(ok, carry_len=L), dict(ok, m=17), dict(ok, m=19),
           dict(ok, skip=-1), dict(ok, raw=0), dict(ok, taps=0), dict(ok, out=0), dict(ok, carry_out=0),
           dict(ok, carry_len=2, m=19, carry_in=0), dict(ok, carry_len=2, m=19, carry_out=ptr(cin)),
           dict(ok, pitch=n - 1), dict(ok, itype=2), dict(ok, rows=0), dict(ok, carry_len=1, skip=1)]
    for d in bad:
        with pytest.raises(ValueError):
            lib().fir_decimate(stream(), d)
    # the wrapper refuses the same before the launch
    big = torch.ones(1026, device="cuda")
    for call in (lambda: HF.fir_decimate(raw, None, 0, 0, taps, 0, out=out),
                 lambda: HF.fir_decimate(raw, None, 0, 0, taps, 65, out=out),
                 lambda: HF.fir_decimate(raw, None, 0, 0, big, D),
                 lambda: HF.fir_decimate(raw, cin, L, 0, taps, D, out=out),
                 lambda: HF.fir_decimate(raw, None, 0, 0, taps, D, out=out, m=17),
                 lambda: HF.fir_decimate(raw, None, 2, 0, taps, D),
                 lambda: HF.fir_decimate(raw, cin, 2, 0, taps, D, carry_out=cin),
                 lambda: HF.fir_decimate(raw.transpose(1, 2), None, 0, 0, taps, D)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        HF.fir_decimate(raw.double(), None, 0, 0, taps, D)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(cout).all() and torch.isnan(cin).all()


# ---------------------------------------------------------------------------------------------------------------
E2E_F, E2E_D, E2E_STRIDE, E2E_CELL, RAW_CHUNKS = 200, 3, (100, 125), (50, 125), (1, 747, 390, 231, 1377)
E2E_T = 3 * 899 + 49  # 900 decimated samples with the default 49 taps
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


def _raw(kind):
    """The 2,746-sample raw streams: ``real`` is noise with a loud patch (the gate has both kinds of window to
    tell apart), ``int16`` integer-valued."""
    g = torch.Generator().manual_seed(3)
    if kind == "int16":
        return torch.randint(-2000, 2001, (E2E_F, E2E_T), generator=g).to(torch.int16)
    raw = torch.randn(E2E_F, E2E_T, generator=g)
    raw[100:, 900:2000] *= 6.0
    return raw


def _offline(model_type):
    """predict_recording(decimate=3) of both raw streams (and gated, Model A) on one kept runner."""
    from mtl_das_pytorch_amd.inference import predict_recording, window_runner
    key = ("off", model_type)
    if key not in _cache:
        m = _model(model_type)
        runner = window_runner(m, model_type, 8, torch.device("cuda"))
        kw = dict(stride=E2E_STRIDE, batch=8, device="cuda", use_engine=True, runner=runner, decimate=E2E_D)
        res = {kind: predict_recording(m, model_type, _raw(kind), **kw) for kind in ("real", "int16")}
        if model_type == "MTL":
            res["gated"] = predict_recording(m, model_type, _raw("real"), **kw, **GATE)
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
        outs.append(live.push(chunk.cuda() if i % 2 else chunk))  # device and host chunks
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
    return order


@pytest.mark.parametrize("kind", ["real", "int16"])
@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_live_decimated_engine_matches_predict_recording(model_type, kind):
    """Raw chunks through LiveRecording(decimate=3): the windows, predictions and probabilities of
    predict_recording(decimate=3) on the whole raw recording, bit-equal (the decimated stream has the same bits
    however it is cut, and the rest is the live path's existing equality); one capture; the map columns against the
    fp64 map of the run's own probabilities within live_map's bound."""
    from mtl_das_pytorch_amd.inference import WINDOW, window_map_reference, window_starts
    off = _offline(model_type)[kind]
    outs = _live(model_type, _raw(kind), RAW_CHUNKS, decimate=E2E_D)
    order = _assert_same_windows(outs, off, ("raw_time_start", "raw_time_stop"))
    assert np.array_equal(off["raw_time_start"], off["positions"][:, 1] * 3)
    assert np.array_equal(off["raw_time_stop"], (off["positions"][:, 1] + 249) * 3 + 49)
    assert len(outs[0]["positions"]) == 0  # one raw sample

    fs, ts = window_starts(E2E_F, WINDOW[0], E2E_STRIDE[0]), window_starts(900, WINDOW[1], E2E_STRIDE[1])
    keys = [k for k in off if k.endswith("_prob")]
    table = np.concatenate([np.concatenate([o[k] for o in outs])[order] for k in keys], 1)
    want = window_map_reference(table, fs, ts, (E2E_F, 900), E2E_CELL)
    got = np.concatenate([o["map_columns"]["class_map"] for o in outs], -1)
    assert outs[-1]["map_columns"]["last"] == 8

    def count(starts, win, length, c):
        return np.array([sum(1 for s in starts if s < min(x + c, length) and s + win > x) for x in range(0, length, c)])
    pairs = count(fs, WINDOW[0], E2E_F, E2E_CELL[0])[:, None] * count(ts, WINDOW[1], 900, E2E_CELL[1])[None]
    bound = (pairs + 3) * 2.0 ** -24
    err = np.abs(got - want)
    print(f"{model_type} {kind} decimated live class map: worst abs err {err.max():.3e}, bound {bound.max():.3e}")
    assert got.shape == want.shape and (err <= bound[None]).all(), err.max()


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_front_end_adds_nothing_but_the_samples(model_type):
    """LiveRecording(decimate=None) on the recording decimated beforehand: the same bits again."""
    from mtl_das_pytorch_amd.inference import decimate_recording
    rec = decimate_recording(_raw("real"), E2E_D, device="cuda")
    assert rec.is_cuda and rec.shape == (1, E2E_F, 900) and rec.dtype == torch.float32
    outs = _live(model_type, rec[0].cpu(), (1, 249, 130, 77, 443))
    _assert_same_windows(outs, _offline(model_type)["real"])
    assert "raw_time_start" not in outs[0]


def test_live_decimated_gated_matches_offline():
    off = _offline("MTL")["gated"]
    assert off["active"].any() and not off["active"].all()
    outs = _live("MTL", _raw("real"), RAW_CHUNKS, decimate=E2E_D, **GATE)
    _assert_same_windows(outs, off, ("active",))
