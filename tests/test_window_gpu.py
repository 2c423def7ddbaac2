"""GPU: resident-recording inference -- the window gather, the probability table and the cell map kernels against
the materialised windows / fp64 references, and predict_recording(windows="resident") end to end against the
materialised path (same model, same engine program)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int16)


def _small():
    """rec [2, 13, 19], window (5, 7), stride (3, 4): 4 x 4 windows, both axes with an end-aligned last window."""
    from mtl_das_pytorch_amd.inference import sliding_windows, window_starts
    rec = torch.randn(2, 13, 19, generator=torch.Generator().manual_seed(0))
    fs, ts = window_starts(13, 5, 3), window_starts(19, 7, 4)
    assert list(fs) == [0, 3, 6, 8] and list(ts) == [0, 4, 8, 12]
    tiles, pos = sliding_windows(rec, window=(5, 7), stride=(3, 4))
    return rec.cuda(), fs, ts, tiles.cuda()


def test_gather_windows_unpacked_matches_gather_batch():
    from mtl_das_pytorch_amd.ops import functional as F
    rec, fs, ts, tiles = _small()
    idx = torch.tensor([0, 15, 6, -1, 9], device="cuda")
    out, lab = F.gather_windows(rec, fs, ts, (5, 7), 5, idx=idx)
    ref, _ = F.gather_batch(tiles, torch.ones(16, 2, dtype=torch.int64, device="cuda"), idx.clamp(min=0))
    assert out.shape == ref.shape == (5, 5, 7, 8)
    valid = [0, 1, 2, 4]
    assert torch.equal(_bits(out[valid]), _bits(ref[valid]))
    assert (out[valid, :, :, :2].float().abs() > 0).all() and (_bits(out[valid, :, :, 2:]) == 0).all()
    assert (_bits(out[3]) == 0).all()  # the -1 row: exactly zero
    assert lab.shape == (5, 2) and (lab == 0).all()


def test_gather_windows_tap_packed_pads_at_the_window_edge():
    """Channel j of pixel (h, w) is x[h - off + j][w] inside the window.  The rows just outside the interior window
    f0 = 3 (recording rows 2 and 8) hold 1e3: padding taken from the recording would show them."""
    from mtl_das_pytorch_amd.inference import sliding_windows, window_starts
    from mtl_das_pytorch_amd.ops import functional as F
    rec = torch.randn(1, 13, 19, generator=torch.Generator().manual_seed(1))
    rec[:, 2] = 1e3
    rec[:, 8] = 1e3
    fs, ts = window_starts(13, 5, 3), window_starts(19, 7, 4)
    tiles = sliding_windows(rec, window=(5, 7), stride=(3, 4))[0].cuda()
    idx = torch.arange(16, device="cuda")
    out, _ = F.gather_windows(rec.cuda(), fs, ts, (5, 7), 16, idx=idx, taps=3, off=1)
    ref, _ = F.gather_batch(tiles, torch.zeros(16, 2, dtype=torch.int64, device="cuda"), idx, taps=3, off=1)
    assert torch.equal(_bits(out), _bits(ref))
    inner = out[4:8].float()  # windows a = 1 (f0 = 3)
    assert (inner[:, 0, :, 0] == 0).all() and (inner[:, 4, :, 2] == 0).all()  # x[-1], x[5] of the window: zero
    assert inner.abs().max() < 100  # and nowhere the 1e3 rows


def test_gather_windows_cursor_form():
    from mtl_das_pytorch_amd.ops import functional as F
    rec, fs, ts, tiles = _small()
    lab = torch.zeros(16, 2, dtype=torch.int64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = [[3, 4, 5, 6], [7, 8, 9, 10], [11, 12, 13, None]]
    for step, rows in enumerate(want):
        cursor.fill_(step)
        out, _ = F.gather_windows(rec, fs, ts, (5, 7), 4, cursor=cursor, lo=3, hi=14)
        ref, _ = F.gather_batch(tiles, lab, torch.tensor([r or 0 for r in rows], device="cuda"))
        for r, n in enumerate(rows):
            if n is None:
                assert (_bits(out[r]) == 0).all()
            else:
                assert torch.equal(_bits(out[r]), _bits(ref[r])), (step, r)
    assert cursor.item() == 2  # the gather reads the cursor, window_probs advances it


def test_window_probs_task_heads_layout():
    """exp of logp[t, r, :k_t], distance | event side by side.  Tolerance 2^-22 relative: expf within 1 ulp
    (2^-23) and the fp32 store of the reference (2^-24)."""
    from mtl_das_pytorch_amd.ops import functional as F
    g = torch.Generator().manual_seed(2)
    logp = torch.full((2, 4, 16), -50.0)
    logp[0] = torch.log_softmax(3 * torch.randn(4, 16, generator=g), 1)
    logp[1, :, :2] = torch.log_softmax(3 * torch.randn(4, 2, generator=g), 1)
    probs = torch.full((9, 18), -7.0, device="cuda")
    idx = torch.tensor([2, -1, 8, 5], device="cuda")
    F.window_probs(logp.cuda(), probs, idx=idx, ncls=[16, 2])
    got = probs.cpu().double()
    want = torch.cat([logp[0].double().exp(), logp[1, :, :2].double().exp()], 1)
    for r, n in enumerate(idx.tolist()):
        if n >= 0:
            rel = ((got[n] - want[r]).abs() / want[r]).max().item()
            print(f"window_probs A row {n}: max rel err {rel:.3e}")
            assert rel <= 2.0 ** -22, rel
    untouched = [n for n in range(9) if n not in (2, 8, 5)]
    assert (probs[untouched] == -7.0).all()
    # rows at or past hi are skipped too
    probs2 = torch.full((9, 18), -7.0, device="cuda")
    F.window_probs(logp.cuda(), probs2, idx=idx, hi=6, ncls=[16, 2])
    assert (probs2[8] == -7.0).all() and torch.equal(probs2[[2, 5]], probs[[2, 5]])


def test_window_probs_joint_softmax_and_cursor():
    """Max-subtracted softmax of 32 logits scaled by 20.  4e-6 absolute: 32 one-ulp terms, the sum and a divide come
    to fewer than 40 * 2^-24 = 2.4e-6 on values <= 1."""
    from mtl_das_pytorch_amd.ops import functional as F
    logits = 20 * torch.randn(4, 32, generator=torch.Generator().manual_seed(3))
    want = torch.softmax(logits.double(), 1)
    probs = torch.full((9, 32), -7.0, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    F.window_probs(logits.cuda(), probs, cursor=cursor, lo=1, hi=7)  # rows 1..4
    assert cursor.item() == 1
    F.window_probs(logits.cuda(), probs, cursor=cursor, lo=1, hi=7)  # rows 5, 6; two padding rows
    assert cursor.item() == 2
    got = probs.cpu().double()
    err = max((got[1:5] - want).abs().max().item(), (got[5:7] - want[:2]).abs().max().item())
    print(f"window_probs C: max abs err {err:.3e}")
    assert err <= 4e-6, err
    assert (probs[[0, 7, 8]] == -7.0).all()


def _map_bound(fs, ts, shape, window, cell):
    """(n + 4) * 2^-23 with n the largest number of windows overlapping one cell, counted here."""
    def most(starts, win, length, c):
        return max(sum(1 for s in starts if s < min(x + c, length) and s + win > x) for x in range(0, length, c))
    n = most(fs, window[0], shape[0], cell[0]) * most(ts, window[1], shape[1], cell[1])
    return (n + 4) * 2.0 ** -23, n


def test_window_map_matches_fp64_and_is_deterministic():
    from mtl_das_pytorch_amd.inference import window_map_reference, window_starts
    from mtl_das_pytorch_amd.ops import functional as F
    shape, win, stride, cell = (23, 41), (5, 8), (3, 5), (4, 7)
    fs, ts = window_starts(shape[0], win[0], stride[0]), window_starts(shape[1], win[1], stride[1])
    probs = torch.rand(len(fs) * len(ts), 3, generator=torch.Generator().manual_seed(4))
    a = F.window_map(probs.cuda(), fs, ts, shape, win, cell)
    b = F.window_map(probs.cuda(), fs, ts, shape, win, cell)
    assert a.shape == (3, 6, 6) and torch.equal(a, b)
    want = window_map_reference(probs.numpy(), fs, ts, shape, cell, win)
    bound, n = _map_bound(fs, ts, shape, win, cell)
    err = np.abs(a.cpu().numpy().astype(np.float64) - want).max()
    print(f"window_map: max abs err {err:.3e}, bound {bound:.3e} (n = {n})")
    assert err <= bound, (err, bound)
    with pytest.raises(ValueError):  # starts that leave rows 5..8 uncovered: those samples have no value
        F.window_map(probs[:5 * len(ts)].cuda(), [0, 9, 12, 15, 18], ts, shape, win, cell)


# ---------------------------------------------------------------------------------------------------------------
STRIDE, BATCH = (10, 50), 32
# an untrained Model A's distance probabilities are nearly flat (top-2 margins around 1e-4): a seed at which at most 2
# of the oracle's 140 windows have a margin under 1e-5
SEED = 1


class _Run:
    pass


_runs = {}


def _e2e(model_type):
    """One model, one recording: the materialised oracle, resident calls on one runner at stride (10, 50), (10, 50)
    again, (100, 350) (3 x 3 windows) and (10, 50), with the growth of the allocator's peak across the last two."""
    if model_type in _runs:
        return _runs[model_type]
    from mtl_das_pytorch_amd.inference import predict_recording, window_runner
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(SEED)
    m = build_model(model_type)
    m.train()  # non-trivial BN running statistics, so eval mode is exercised
    with torch.no_grad():
        m(torch.randn(8, 1, 100, 250))
    m.eval()
    rec = torch.randn(230, 700)
    r = _Run()
    r.rec = rec
    r.oracle = predict_recording(m, model_type, rec, stride=STRIDE, batch=BATCH, device="cuda", use_engine=True,
                                 windows="materialize")
    runner = window_runner(m, model_type, BATCH, torch.device("cuda"))

    def grown(stride):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = predict_recording(m, model_type, rec, stride=stride, batch=BATCH, device="cuda", use_engine=True,
                                windows="resident", runner=runner)
        torch.cuda.synchronize()
        return res, torch.cuda.max_memory_allocated() - base

    r.res, r.grow_first = grown(STRIDE)
    r.res2, _ = grown(STRIDE)
    # both measured calls start from a runner that holds another recording's buffers and capture their graph anew
    r.sparse, r.grow_sparse = grown((100, 350))
    r.res3, r.grow_dense = grown(STRIDE)
    runner.close()
    # the call as infer.py makes it: no runner, the model lowered, captured and released inside
    r.plain = predict_recording(m, model_type, rec, stride=STRIDE, batch=BATCH, device="cuda", use_engine=True)
    _runs[model_type] = r
    return r


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_resident_matches_materialized(model_type):
    r = _e2e(model_type)
    assert len(r.oracle["positions"]) == 140 and np.array_equal(r.res["positions"], r.oracle["positions"])
    under = np.zeros(140, dtype=bool)
    keys = [k for k in r.oracle if k.endswith("_prob")]
    assert keys and set(r.res) == set(r.oracle) == set(r.plain)
    for k in r.res:  # windows="resident" is the engine's default, with a runner of its own
        assert np.array_equal(r.plain[k], r.res[k]), k
    for k in keys:
        err = np.abs(r.res[k].astype(np.float64) - r.oracle[k]).max()
        print(f"{model_type} {k}: max abs diff {err:.3e}")
        assert r.res[k].shape == r.oracle[k].shape and err <= 4e-6, (k, err)
        top = np.sort(r.oracle[k], 1)
        low = top[:, -1] - top[:, -2] <= 1e-5
        under |= low
        name = k[:-5]
        assert np.array_equal(r.res[f"{name}_pred"][~low], r.oracle[f"{name}_pred"][~low])
    print(f"{model_type}: {int(under.sum())} windows under the 1e-5 margin")
    assert under.sum() <= 2
    if model_type == "multi_classifier":  # decoded from the joint prediction
        for k in ("distance_pred", "event_pred"):
            assert np.array_equal(r.res[k][~under], r.oracle[k][~under])


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_resident_memory_does_not_grow_with_the_window_count(model_type):
    """140 windows at stride (10, 50) against 9 at (100, 350) (starts 0, 100, 130 x 0, 350, 450): the materialised
    stack alone would add 13 MB."""
    r = _e2e(model_type)
    assert len(r.sparse["positions"]) == 9
    print(f"{model_type}: peak growth {r.grow_dense} B (140 windows), {r.grow_sparse} B (9 windows); the runner's "
          f"first call {r.grow_first} B")
    assert abs(r.grow_dense - r.grow_sparse) < 2 ** 20


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_resident_is_repeatable(model_type):
    """The second call replays the first call's graph from a reset cursor: bitwise the same table (a warm-up that was
    not rolled back, or a cursor that was not reset, shifts or drops batches)."""
    r = _e2e(model_type)
    for k in r.res:
        assert np.array_equal(r.res[k], r.res2[k]), k
        assert np.array_equal(r.res[k], r.res3[k]), k  # and after another recording's geometry in between
    key = "joint_prob" if model_type == "multi_classifier" else "event_prob"
    assert (np.abs(r.res[key].sum(1) - 1) < 1e-5).all()  # every row was written, the padded tail's included


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_prediction_map_on_device_matches_numpy(model_type):
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map, window_starts
    r = _e2e(model_type)
    shape, cell = tuple(r.rec.shape), (20, 100)
    fs, ts = window_starts(shape[0], WINDOW[0], STRIDE[0]), window_starts(shape[1], WINDOW[1], STRIDE[1])
    if model_type == "multi_classifier":
        table = r.res["joint_prob"]
    else:
        table = np.concatenate([r.res["distance_prob"], r.res["event_prob"]], 1)
    dev = prediction_map(torch.from_numpy(table).cuda(), fs, ts, shape, cell)
    ref = prediction_map(table, fs, ts, shape, cell)
    bound, n = _map_bound(fs, ts, shape, WINDOW, cell)
    # the kernel's own output, every class of the table
    from mtl_das_pytorch_amd.inference import window_map_reference
    from mtl_das_pytorch_amd.ops import functional as F
    raw = F.window_map(torch.from_numpy(table).cuda(), fs, ts, shape, WINDOW, cell).cpu().numpy().astype(np.float64)
    err = np.abs(raw - window_map_reference(table, fs, ts, shape, cell)).max()
    print(f"{model_type} class map: max abs err {err:.3e}, bound {bound:.3e} (n = {n})")
    assert err <= bound, err
    assert dev["event_map"].shape == (2, 12, 7) and dev["distance_map"].shape == (16, 12, 7)
    for k in ("event_map", "distance_map"):
        err = np.abs(dev[k].astype(np.float64) - ref[k]).max()
        print(f"{model_type} {k}: max abs err {err:.3e}, bound {bound:.3e} (n = {n})")
        assert err <= bound, (k, err)
    assert np.abs(dev["event_map"].sum(0) - 1).max() < 1e-4
    assert dev["distance_mean_m"].shape == (12, 7)
