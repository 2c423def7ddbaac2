"""GPU: the activity gate of resident-recording inference (csrc/gate.hip) -- the window power against the fp64
definition, the ordered selection against np.flatnonzero, the selected forms of the window gather and the probability
store against their index forms, and predict_recording(gate_db=...) end to end against the ungated resident path."""
import numpy as np
import pytest
import torch

import gate_ref as G

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int16)


# ---- window_power ---------------------------------------------------------------------------------------------
def _power_case(rec, fs, ts, window):
    """|err| <= 2^-23 P: the value has one fp32 rounding on the store (2^-24 P); the fp64 accumulation of at most
    25000 terms is orders of magnitude below that.  Two launches are bitwise equal."""
    from mtl_das_pytorch_amd.inference import window_power_reference
    from mtl_das_pytorch_amd.ops import functional as F
    want = window_power_reference(rec, fs, ts, window)
    dev = torch.from_numpy(rec).cuda()
    a = F.window_power(dev, fs, ts, window)
    b = F.window_power(dev, fs, ts, window)
    assert a.shape == (len(fs) * len(ts),) and a.dtype == torch.float32
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rel = np.abs(a.cpu().numpy().astype(np.float64) - want) / want
    print(f"window_power {rec.shape} window {window}: max rel err {rel.max():.3e} (bound {2.0 ** -23:.3e})")
    assert (rel <= 2.0 ** -23).all(), rel.max()


@pytest.mark.parametrize("C", [1, 2])
def test_window_power_small_window_with_offset(C):
    """Unit noise on an offset of 50 per channel: an uncentred sum of squares (2500 + 1 in fp32 terms, or
    E[x^2] - E[x]^2) would lose the signal.  Window (12, 40) = 480 elements, no multiple of the block; the starts
    include the end-aligned ones (18 of 30 rows, 90 of 130 columns)."""
    from mtl_das_pytorch_amd.inference import window_starts
    rec = np.random.default_rng(10 + C).standard_normal((C, 30, 130)).astype(np.float32)
    rec += (50.0 * (1 + np.arange(C, dtype=np.float32)))[:, None, None]
    fs, ts = window_starts(30, 12, 5), window_starts(130, 40, 16)
    assert list(fs) == [0, 5, 10, 15, 18] and list(ts) == [0, 16, 32, 48, 64, 80, 90]
    _power_case(rec, fs, ts, (12, 40))


def test_window_power_model_window_on_the_fixture():
    """The models' (100, 250) window: 25000 elements, 98 loop trips per thread."""
    from mtl_das_pytorch_amd.inference import WINDOW
    rec, fs, ts, _ = G.fixture()
    _power_case(rec[None].copy(), fs, ts, WINDOW)


# ---- select_windows -------------------------------------------------------------------------------------------
NT = 7  # windows per fiber start: divides neither the wave nor the block


def _select_case(power, floor, gate_db, lo, hi):
    from mtl_das_pytorch_amd.ops import functional as F
    N = len(power)
    # the kernel's threshold: one fp32 multiply of the start's floor and the fp32 ratio
    thr = floor[np.arange(N) // NT] * np.float32(F.gate_ratio(gate_db))
    assert thr.dtype == np.float32
    want = ~(power < thr)
    want[:lo] = False
    want[hi:] = False
    sel = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    s, count, active = F.select_windows(torch.from_numpy(power).cuda(), torch.from_numpy(floor).cuda(), gate_db, NT,
                                        lo, hi, sel=sel)
    assert s is sel and count.dtype == torch.int64 and active.dtype == torch.uint8
    idx = np.flatnonzero(want)
    assert count.item() == len(idx), (N, lo, hi, count.item(), len(idx))
    got = sel.cpu().numpy()
    assert np.array_equal(got[:len(idx)], idx)  # exact and ascending
    assert (got[len(idx):] == -1).all()         # the rest keeps its prefill
    assert np.array_equal(active.cpu().numpy(), want.astype(np.uint8))
    return len(idx)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 5000, 70001])
def test_select_windows_matches_flatnonzero(N):
    """70001 windows are 274 blocks: more than one block's worth of block counts.  Patterns: all, none, Bernoulli 1/2
    (with powers exactly on the threshold, which are active), only the last window; the whole range and
    [7, N - 3)."""
    rng = np.random.default_rng(N)
    floor = (0.5 + rng.random((N + NT - 1) // NT)).astype(np.float32)
    gate_db = 3.0
    from mtl_das_pytorch_amd.ops.functional import gate_ratio
    thr = floor[np.arange(N) // NT] * np.float32(gate_ratio(gate_db))
    patterns = {"all": np.ones(N, bool), "none": np.zeros(N, bool), "half": rng.random(N) < 0.5,
                "last": np.arange(N) == N - 1}
    ranges = [(0, N)] + ([(7, N - 3)] if N > 10 else [])
    for name, on in patterns.items():
        power = np.where(on, thr * np.float32(1.5), thr * np.float32(0.75)).astype(np.float32)
        if name == "half":
            edge = on & (rng.random(N) < 0.25)
            power[edge] = thr[edge]  # not below the threshold: active
        for lo, hi in ranges:
            n = _select_case(power, floor, gate_db, lo, hi)
            expect = int(on[lo:hi].sum())
            assert n == expect, (name, lo, hi, n, expect)


def test_select_windows_never_hides_a_nan():
    N = 300
    floor = np.ones((N + NT - 1) // NT, dtype=np.float32)
    power = np.full(N, 0.25, dtype=np.float32)
    power[[0, 129, 299]] = np.nan
    assert _select_case(power, floor, 0.0, 0, N) == 3
    assert _select_case(power, floor, 0.0, 7, N - 3) == 1


# ---- selected gather and probability store --------------------------------------------------------------------
B, COUNT = 4, 5
# capacity 9: the entries past the count are window numbers too, so a launch that read them would show
SEL = [3, 0, 15, 6, 9, 1, 2, 4, 5]


@pytest.mark.parametrize("taps,off,C", [(0, 0, 2), (3, 1, 1)])
def test_gather_windows_selected_form(taps, off, C):
    from mtl_das_pytorch_amd.inference import window_starts
    from mtl_das_pytorch_amd.ops import functional as F
    rec = torch.randn(C, 13, 19, generator=torch.Generator().manual_seed(0)).cuda()
    fs, ts = window_starts(13, 5, 3), window_starts(19, 7, 4)  # 4 x 4 windows
    sel = torch.tensor(SEL, device="cuda")
    count = torch.tensor([COUNT], device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    kw = dict(taps=taps, off=off)
    first, lab = F.gather_windows(rec, fs, ts, (5, 7), B, cursor=cursor, sel=sel, count=count, **kw)
    ref, _ = F.gather_windows(rec, fs, ts, (5, 7), B, idx=sel[0:4].contiguous(), **kw)
    assert torch.equal(_bits(first), _bits(ref)) and (first.float().abs().sum((1, 2, 3)) > 0).all()
    assert (lab == 0).all() and cursor.item() == 0  # the gather reads the cursor, the store advances it
    cursor.fill_(1)
    second, _ = F.gather_windows(rec, fs, ts, (5, 7), B, cursor=cursor, sel=sel, count=count, **kw)
    ref, _ = F.gather_windows(rec, fs, ts, (5, 7), B, idx=torch.tensor([SEL[4], -1, -1, -1], device="cuda"), **kw)
    assert torch.equal(_bits(second[0]), _bits(ref[0]))
    assert (_bits(second[1:]) == 0).all()  # past the count: padding, whatever sel holds there
    cursor.fill_(3)  # past the capacity: nothing is read
    third, _ = F.gather_windows(rec, fs, ts, (5, 7), B, cursor=cursor, sel=sel, count=count, **kw)
    assert (_bits(third) == 0).all()
    with pytest.raises(ValueError):
        F.gather_windows(rec, fs, ts, (5, 7), B, idx=sel[0:4].contiguous(), sel=sel, count=count)


def _store_case(src, K, ncls):
    """Two replays write exactly the five selected rows, the values of the index form bitwise; the cursor ends
    at 2."""
    from mtl_das_pytorch_amd.ops import functional as F
    sel = torch.tensor(SEL, device="cuda")
    count = torch.tensor([COUNT], device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    probs = torch.full((16, K), -7.0, device="cuda")
    F.window_probs(src, probs, cursor=cursor, sel=sel, count=count, ncls=ncls)
    assert cursor.item() == 1
    F.window_probs(src, probs, cursor=cursor, sel=sel, count=count, ncls=ncls)
    assert cursor.item() == 2
    want = torch.full((16, K), -7.0, device="cuda")
    F.window_probs(src, want, idx=torch.tensor(SEL[0:4], device="cuda"), ncls=ncls)
    F.window_probs(src, want, idx=torch.tensor([SEL[4], -1, -1, -1], device="cuda"), ncls=ncls)
    assert torch.equal(probs.view(torch.int32), want.view(torch.int32))
    written = sorted(SEL[:COUNT])
    assert (probs[[n for n in range(16) if n not in written]] == -7.0).all()
    assert (probs[written] >= 0).all() and (probs[written].sum(1) > 0.99).all()


def test_window_probs_selected_form_task_heads():
    g = torch.Generator().manual_seed(2)
    logp = torch.full((2, B, 16), -50.0)
    logp[0] = torch.log_softmax(3 * torch.randn(B, 16, generator=g), 1)
    logp[1, :, :2] = torch.log_softmax(3 * torch.randn(B, 2, generator=g), 1)
    _store_case(logp.cuda(), 18, [16, 2])


def test_window_probs_selected_form_softmax():
    logits = 20 * torch.randn(B, 32, generator=torch.Generator().manual_seed(3))
    _store_case(logits.cuda(), 32, None)


# ---- end to end -----------------------------------------------------------------------------------------------
BATCH = 32
SEED = 1  # as test_window_gpu.py


class _Run:
    pass


_runs = {}


def _e2e(model_type):
    """One model, one runner, the fixture recording: the ungated resident result, the gate that keeps everything,
    and the 3 dB gate twice -- with the infer_step calls and the captures of each call."""
    if model_type in _runs:
        return _runs[model_type]
    from mtl_das_pytorch_amd.inference import predict_recording, window_runner
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(SEED)
    m = build_model(model_type)
    m.train()  # non-trivial BN running statistics
    with torch.no_grad():
        m(torch.randn(8, 1, 100, 250))
    m.eval()
    rec = torch.from_numpy(G.fixture()[0].copy())
    runner = window_runner(m, model_type, BATCH, torch.device("cuda"))
    steps = [0]
    infer_step = runner.infer_step

    def counted():
        steps[0] += 1
        infer_step()

    runner.infer_step = counted

    def call(**gate):
        steps[0] = 0
        res = predict_recording(m, model_type, rec, stride=G.STRIDE, batch=BATCH, device="cuda", use_engine=True,
                                windows="resident", runner=runner, **gate)
        return res, steps[0], runner.captures

    r = _Run()
    r.model = m
    r.plain = call()
    r.keep = call(gate_db=-100.0, noise_floor=1.0)
    r.gated = call(gate_db=G.GATE_DB, noise_floor=1.0)
    r.again = call(gate_db=G.GATE_DB, noise_floor=1.0)
    r.auto = call(gate_db=G.GATE_DB, noise_floor="auto")
    runner.close()
    _runs[model_type] = r
    return r


MODELS = ["MTL", "multi_classifier"]


@pytest.mark.parametrize("model_type", MODELS)
def test_gate_that_keeps_everything_changes_nothing(model_type):
    """-100 dB under a floor of 1: every window is active and the batches are those of the ungated call."""
    r = _e2e(model_type)
    plain, keep = r.plain[0], r.keep[0]
    assert keep["active"].all() and r.keep[1] == r.plain[1] == 5
    assert set(keep) == set(plain) | {"active", "power_db"}
    for k in plain:
        assert np.array_equal(keep[k], plain[k]), k
    power = G.fixture()[3]
    assert np.abs(keep["power_db"] - 10 * np.log10(power)).max() < 1e-5  # 2^-23 relative is 5e-7 dB


@pytest.mark.parametrize("model_type", MODELS)
def test_gated_recording_skips_the_quiet_windows(model_type):
    r = _e2e(model_type)
    want = G.fixture_flags(1.0)
    assert want.sum() == 60
    plain, (res, steps, captures) = r.plain[0], r.gated
    assert np.array_equal(res["active"], want)
    assert steps == 2 and r.plain[1] == 5  # ceil(60 / 32) replays against ceil(140 / 32)
    for k in [k for k in res if k.endswith("_pred")]:
        assert (res[k][~want] == -1).all() and (res[k][want] >= 0).all(), k
    for k in [k for k in res if k.endswith("_prob")]:
        assert (res[k][~want] == 0).all(), k
        diff = np.abs(res[k][want].astype(np.float64) - plain[k][want]).max()
        print(f"{model_type} {k}: active rows against the ungated rows, max abs diff {diff:.3e}")
        # Other batch neighbours, the same window: eval BN uses running statistics and every output pixel of the
        # convolutions is accumulated in an order that does not depend on its batch row, so the rows are equal --
        # measured 0 on the MI355X for both models; the bound for two paths to the same probabilities is 4e-6
        # (test_window_gpu.py)
        assert diff == 0, (k, diff)
    # the second gated call replays the first one's graph and gives the same bits
    again, steps2, captures2 = r.again
    assert captures2 == captures and steps2 == 2
    for k in res:
        assert np.array_equal(res[k], again[k], equal_nan=k == "power_db"), k


@pytest.mark.parametrize("model_type", MODELS)
def test_gated_recording_auto_floor(model_type):
    """The floor computed on the device (torch.sort) selects what the fp64 lower median selects; the selection is
    device data, so the graph of the fixed-floor calls serves it."""
    r = _e2e(model_type)
    want = G.fixture_flags("auto")
    res, steps, captures = r.auto
    assert np.array_equal(res["active"], want)
    assert steps == -(-int(want.sum()) // BATCH) and captures == r.gated[2]


def test_gated_materialized_windows_on_the_engine():
    """windows="materialize" honours the gate by the fp64 reference and stacks only the active windows: the flags of
    the resident path, and its probabilities within the bound for two paths to the same probabilities (4e-6,
    test_window_gpu.py)."""
    from mtl_das_pytorch_amd.inference import predict_recording
    r = _e2e("MTL")
    rec = torch.from_numpy(G.fixture()[0].copy())
    res = predict_recording(r.model, "MTL", rec, stride=G.STRIDE, batch=BATCH, device="cuda", use_engine=True,
                            windows="materialize", gate_db=G.GATE_DB, noise_floor=1.0)
    want = r.gated[0]
    assert set(res) == set(want) and np.array_equal(res["active"], want["active"])
    for k in ("distance_prob", "event_prob"):
        err = np.abs(res[k].astype(np.float64) - want[k]).max()
        print(f"materialised against resident, gated, {k}: max abs diff {err:.3e}")
        assert err <= 4e-6 and (res[k][~res["active"]] == 0).all(), (k, err)
    assert (res["event_pred"][~res["active"]] == -1).all()


@pytest.mark.parametrize("model_type", MODELS)
def test_gated_prediction_map_on_device_matches_numpy(model_type):
    from test_window_gpu import _map_bound
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map, window_map_reference
    from mtl_das_pytorch_amd.ops import functional as F
    res = _e2e(model_type).gated[0]
    _, fs, ts, _ = G.fixture()
    shape, cell = (230, 700), (20, 100)
    if model_type == "multi_classifier":
        table = res["joint_prob"]
    else:
        table = np.concatenate([res["distance_prob"], res["event_prob"]], 1)
    active = res["active"]
    # the K + 1 class map before the division: the kernel against fp64
    full = np.concatenate([table, active[:, None].astype(np.float32)], 1)
    raw = F.window_map(torch.from_numpy(full).cuda(), fs, ts, shape, WINDOW, cell).cpu().numpy().astype(np.float64)
    bound, n = _map_bound(fs, ts, shape, WINDOW, cell)
    err = np.abs(raw - window_map_reference(full, fs, ts, shape, cell)).max()
    print(f"{model_type} gated class map (K + 1 = {full.shape[1]}): max abs err {err:.3e}, bound {bound:.3e} (n = {n})")
    assert err <= bound, err
    dev = prediction_map(torch.from_numpy(table).cuda(), fs, ts, shape, cell, active=active)
    ref = prediction_map(table, fs, ts, shape, cell, active=active)
    assert set(dev) == set(ref) and "activity_map" in dev
    assert np.abs(dev["activity_map"] - ref["activity_map"]).max() <= bound
    empty = ref["activity_map"] == 0
    assert empty.any() and not empty.all()
    for k in ("event_map", "distance_map", "distance_mean_m"):
        assert np.array_equal(np.isnan(dev[k]), np.isnan(ref[k])), k
        assert np.array_equal(np.isnan(ref[k]), np.broadcast_to(empty, ref[k].shape)), k
    heard = ~empty
    assert np.abs(dev["event_map"][:, heard].sum(0) - 1).max() < 1e-4  # only active windows speak, and they sum to 1
