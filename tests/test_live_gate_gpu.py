"""GPU: the activity gate of a growing recording (csrc/live_gate.hip) -- the ring's window powers against window_power
on the linear recording (bitwise), the running floor against the fp64 reference (a selection: exact), the live
selection against np.flatnonzero, the selected ring gather and probability store against their index forms, the
launchers' refusals, and LiveRecording(gate_db=...) on the engine end to end against predict_recording, the fp64
references and the ungated live run.

Kernel tests: test_live_gpu.py's geometry -- window 5 x 7, F = 9, fiber starts 0, 2, 4, time stride 3, batch 4, chunks
1, 3, 9, 2, 8 = 23 samples: time starts 0, 3, .., 15 and the end-aligned 16.  End to end: test_live_gate.py's fixture
(gate_ref's recording cut to T = 690, stride (10, 50), 3 dB; 10 x 14 windows)."""
import numpy as np
import pytest
import torch

import gate_ref as G

pytestmark = pytest.mark.gpu

WIN, F_, SF, ST, B = (5, 7), 9, 2, 3, 4
CHUNKS = (1, 3, 9, 2, 8)
T_ = sum(CHUNKS)
TOTAL, AVAIL, NEXT, JEND, TEND = range(5)
NF = 3


def _i32(t):
    return t.contiguous().view(torch.int32)


def _geometry():
    from mtl_das_pytorch_amd.inference import window_starts
    fs, ts = window_starts(F_, WIN[0], SF), window_starts(T_, WIN[1], ST)
    assert list(fs) == [0, 2, 4] and list(ts) == [0, 3, 6, 9, 12, 15, 16]
    return fs, ts


def _pieces(n, step):
    return [min(step, n - i) for i in range(0, n, step)]


def _guarded(n, fill, dtype=torch.float32, guard=8):
    """A buffer of n entries followed by sentinels: (whole, the view the launch gets)."""
    whole = torch.full((n + guard,), fill, dtype=dtype, device="cuda")
    return whole, whole[:n]


def _same(got, want):
    """fp32 arrays equal as values, a NaN equal to a NaN."""
    return np.array_equal(got, want, equal_nan=True)


# ---- ring_window_power ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [16, 11])
@pytest.mark.parametrize("C", [1, 3])
def test_ring_window_power_has_the_bits_of_the_linear_recording(R, C):
    """After every append the new windows' powers, read through the ring (NaN before it is written), are bit-equal to
    window_power on the whole linear recording; the power ring holds 5 of the 7 time indices, so it wraps."""
    from mtl_das_pytorch_amd.ops import functional as HF
    fs, ts = _geometry()
    nt, jcap = len(ts), 5
    full = torch.randn(C, F_, T_, generator=torch.Generator().manual_seed(7)).cuda()
    full[:, 4:] += 30.0  # an offset: an uncentred sum would lose the signal
    want = HF.window_power(full, fs, ts, WIN).view(NF, nt)  # [a][j]
    ring = torch.full((C, F_, R), float("nan"), device="cuda")
    state = HF.live_state("cuda")
    whole, power = _guarded(jcap * NF, -3.0)
    total = done = straddle = checked = 0

    def check(j0, j1):
        nonlocal straddle, checked
        HF.ring_window_power(ring, state, fs, ST, WIN, power, jcap, j0 * NF, j1 * NF)
        for j in range(j0, j1):
            got = power[(j % jcap) * NF:(j % jcap + 1) * NF]
            assert torch.equal(_i32(got), _i32(want[:, j])), (R, C, j)
            straddle += int(int(ts[j]) % R + WIN[1] > R)
            checked += 1
        assert (whole[jcap * NF:] == -3.0).all()

    for n in CHUNKS:
        for m in _pieces(n, R - WIN[1]):
            HF.ring_append(ring, state, full[:, :, total:total + m].contiguous(), NF, ST, WIN[1])
            total += m
            nj = (total - WIN[1]) // ST + 1 if total >= WIN[1] else 0
            check(done, nj)
            done = nj
    HF.ring_append(ring, state, None, NF, ST, WIN[1], flush=True)
    check(done, done + 1)  # the end-aligned index
    assert checked == nt and straddle >= 1 and not torch.isnan(power).any()
    # a window that has not arrived has no power: NaN (which the selection keeps), not a read of what is not there
    before = power.clone()
    HF.ring_window_power(ring, state, fs, ST, WIN, power, jcap, nt * NF, (nt + 1) * NF)
    rows = slice((nt % jcap) * NF, (nt % jcap + 1) * NF)
    assert torch.isnan(power[rows]).all()
    power[rows] = before[rows]
    assert torch.equal(_i32(power), _i32(before)) and state.tolist()[NEXT] == 0


# ---- running_floor --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [1, 3])
@pytest.mark.parametrize("warmup", [1, 2])
def test_running_floor_is_the_reference_exactly(history, warmup):
    """9 time indices in pieces of 1, 2, 2, 1, 2, 1 through a power ring of history - 1 + 2 indices (it wraps): the
    floor is one of the fp32 powers (or 0), so it equals the fp64 reference of those powers exactly.  A tied pair, a
    triple and one NaN are among them."""
    from mtl_das_pytorch_amd.inference import running_floor_reference
    from mtl_das_pytorch_amd.ops import functional as HF
    nj, jcap = 9, history - 1 + 2
    p = np.random.default_rng(5).random((nj, NF)).astype(np.float32)
    p[4, 1] = np.nan
    p[2, 0] = p[3, 0]
    p[6, 2] = p[5, 2] = p[4, 2]
    whole_p, power = _guarded(jcap * NF, -3.0)
    whole_f, floor = _guarded(jcap * NF, -4.0)
    if warmup > history:
        with pytest.raises(ValueError):
            HF.running_floor(power, floor, NF, jcap, 0, NF, history, warmup)
        assert (whole_f == -4.0).all()
        return
    want = running_floor_reference(p.astype(np.float64).reshape(-1), NF, history, warmup).astype(np.float32)
    j0 = zeros = nans = 0
    for m in (1, 2, 2, 1, 2, 1):
        for j in range(j0, j0 + m):
            power[(j % jcap) * NF:(j % jcap + 1) * NF] = torch.from_numpy(p[j]).cuda()
        HF.running_floor(power, floor, NF, jcap, j0 * NF, (j0 + m) * NF, history, warmup)
        for j in range(j0, j0 + m):
            got = floor[(j % jcap) * NF:(j % jcap + 1) * NF].cpu().numpy()
            assert _same(got, want[j]), (history, warmup, j, got, want[j])
            zeros += int((got == 0).sum())
            nans += int(np.isnan(got).sum())
        j0 += m
    assert j0 == nj and zeros == NF * (warmup - 1) and nans == int(history == 1)
    assert (whole_p[jcap * NF:] == -3.0).all() and (whole_f[jcap * NF:] == -4.0).all()
    with pytest.raises(ValueError):  # three indices need history - 1 + 3 rows
        HF.running_floor(power, floor, NF, jcap, 0, 3 * NF, history, warmup)


# ---- live_select ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jcap,j0,j1", [(4, 2, 5), (200, 0, 200), (200, 150, 340)])
def test_live_select_matches_flatnonzero(jcap, j0, j1):
    """The flags of [n0, n1) by the kernel's own rule (one fp32 multiply), sel[:count] against flatnonzero, everything
    around it untouched; 600 windows are three blocks; (150, 340) wraps the rings."""
    from mtl_das_pytorch_amd.ops import functional as HF
    K, gate_db = 4, 3.0
    n0, n1, n = j0 * NF, j1 * NF, jcap * NF
    rng = np.random.default_rng(jcap + j0)
    p = rng.random(n).astype(np.float32)
    f = (0.2 + 0.4 * rng.random(n)).astype(np.float32)
    f[rng.random(n) < 0.1] = 0.0   # no floor yet: active
    p[rng.random(n) < 0.05] = np.nan  # never hidden
    edge = rng.random(n) < 0.1
    p[edge] = (f * np.float32(HF.gate_ratio(gate_db)))[edge]  # on the threshold: not below it, active
    rows = np.asarray([(w // NF % jcap) * NF + w % NF for w in range(n0, n1)])
    p[rows[1]], f[rows[2]], p[rows[4]], f[rows[4]] = np.nan, 0.0, 0.1, 0.5  # each kind is in the range
    want = ~(p[rows] < f[rows] * np.float32(HF.gate_ratio(gate_db)))
    assert np.isnan(p[rows]).any() and want[np.isnan(p[rows])].all() and want[f[rows] == 0].all() and not want.all()
    power, floor = torch.from_numpy(p).cuda(), torch.from_numpy(f).cuda()
    whole_a, active = _guarded(n, 9, torch.uint8)
    whole_s, sel = _guarded(n1 - n0 + 5, -1, torch.int64)
    table = torch.full((n + 2, K + 1), 5.0, device="cuda")
    state = HF.live_state("cuda")
    state[AVAIL] = n1
    state[TOTAL] = 10 ** 6
    cursor, count = HF.live_gate_state("cuda")
    cursor.fill_(7)
    HF.live_select(power, floor, active, table, state, sel, count, cursor, gate_db, NF, jcap, n0, n1)
    idx = np.flatnonzero(want) + n0
    assert count.item() == len(idx) and cursor.item() == 0
    assert state.tolist() == [10 ** 6, n1, n1, -1, 0]
    got = whole_s.cpu().numpy()
    assert np.array_equal(got[:len(idx)], idx) and (got[len(idx):] == -1).all()
    act = whole_a.cpu().numpy()
    outside = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(act[rows], want.astype(np.uint8)) and (act[outside] == 9).all() and (act[n:] == 9).all()
    t = table.cpu().numpy()
    assert (t[rows] == 0).all() and (t[outside] == 5.0).all() and (t[n:] == 5.0).all()
    assert len(outside) == n - (n1 - n0)
    # a window past avail cannot be evaluated: it is not selected
    state[AVAIL] = n1 - NF
    HF.live_select(power, floor, active, table, state, sel, count, cursor, gate_db, NF, jcap, n0, n1)
    assert count.item() == int(want[:-NF].sum())


# ---- the selected ring gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [16, 11])
@pytest.mark.parametrize("C,taps,off", [(1, 3, 1), (3, 0, 0)])
def test_selected_ring_gather_matches_linear_gather(R, C, taps, off):
    """13 samples in the ring (R = 11: wrapped, the window at 6 straddles the wrap): six selected windows in batches of
    4 against gather_windows (idx form) on the linear recording; the entries past the count are window numbers too."""
    from mtl_das_pytorch_amd.ops import functional as HF
    fs, ts = _geometry()
    nt = len(ts)
    full = torch.randn(C, F_, T_, generator=torch.Generator().manual_seed(7)).cuda()
    ring = torch.full((C, F_, R), float("nan"), device="cuda")
    state = HF.live_state("cuda")
    total = 0
    for n in (1, 3, 9):
        for m in _pieces(n, R - WIN[1]):
            HF.ring_append(ring, state, full[:, :, total:total + m].contiguous(), NF, ST, WIN[1])
            total += m
    assert state.tolist()[:2] == [13, 9]  # time indices 0, 1, 2; with R = 11 index 0 has left the ring
    order = [7, 3, 5, 8, 4, 6, 3, 5] if R == 11 else [7, 2, 5, 0, 8, 3, 1, 4]
    assert 6 % R + WIN[1] > R or R == 16
    sel = torch.tensor(order, device="cuda")
    cursor, count = HF.live_gate_state("cuda")
    count.fill_(6)  # no multiple of B
    for cur, valid in ((0, 4), (1, 2), (2, 0)):
        cursor.fill_(cur)
        out, lab = HF.gather_windows_ring(ring, state, fs, ST, WIN, B, taps=taps, off=off, sel=sel, count=count,
                                          cursor=cursor)
        rows = [(w % NF) * nt + w // NF for w in order[cur * B:cur * B + valid]] + [-1] * (B - valid)
        ref, _ = HF.gather_windows(full, fs, ts, WIN, B, idx=torch.tensor(rows, device="cuda"), taps=taps, off=off)
        assert not torch.isnan(out.float()).any()
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (R, cur)
        assert (out[valid:].view(torch.int16) == 0).all() and (lab == 0).all()
        assert (out[:valid].float().abs().sum((1, 2, 3)) > 0).all()
        assert cursor.item() == cur and state.tolist()[NEXT] == 0  # the gather reads the counters


# ---- the selected probability store ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["softmax", "logp"])
def test_live_probs_sel_fills_the_gated_table(form):
    """Jcap = 2: the rows of time indices 0, 1 are recycled by 2, 3.  Evaluated rows hold window_probs' bits and a 1 in
    column K; a recycled row whose earlier window was active and whose new one is quiet is all zero."""
    from mtl_das_pytorch_amd.ops import functional as HF
    jcap, gate_db = 2, 0.0
    K = 5 if form == "softmax" else 18
    g = torch.Generator().manual_seed(11)
    n = jcap * NF
    table = torch.full((n + 2, K + 1), -7.0, device="cuda")
    floor = torch.ones(n, device="cuda")
    power = torch.empty(n, device="cuda")
    active = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sel = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    state = HF.live_state("cuda")
    cursor, count = HF.live_gate_state("cuda")
    was_active = np.zeros(n, dtype=bool)
    recycled_quiet = 0
    # per piece: the powers of its two time indices (>= 1: active)
    for piece, pw in enumerate(([2, 2, 0.5, 2, 2, 2], [0.5, 2, 2, 0.5, 0.5, 2])):
        n0, n1 = piece * n, (piece + 1) * n
        state[AVAIL] = n1
        power.copy_(torch.tensor(pw))
        HF.live_select(power, floor, active, table, state, sel, count, cursor, gate_db, NF, jcap, n0, n1)
        on = np.asarray(pw) >= 1
        chosen = [n0 + i for i in np.flatnonzero(on)]
        assert count.item() == len(chosen) and sel[:len(chosen)].tolist() == chosen
        want = torch.zeros(n, K, device="cuda")
        for cur in range(-(-len(chosen) // B)):
            if form == "softmax":
                src, ncls = (8 * torch.randn(B, K, generator=g)).cuda(), None
            else:
                logp = torch.full((2, B, 16), -50.0)
                logp[0] = torch.log_softmax(3 * torch.randn(B, 16, generator=g), 1)
                logp[1, :, :2] = torch.log_softmax(3 * torch.randn(B, 2, generator=g), 1)
                src, ncls = logp.cuda(), [16, 2]
            HF.live_probs(src, table, state, NF, jcap, ncls=ncls, sel=sel, count=count, cursor=cursor)
            assert cursor.item() == cur + 1
            batch = chosen[cur * B:(cur + 1) * B]
            rows = [w - n0 for w in batch] + [-1] * (B - len(batch))  # row (j mod 2) * nf + a = n - n0
            HF.window_probs(src, want, idx=torch.tensor(rows, device="cuda"), ncls=ncls)
        t, on_t = table.cpu(), torch.from_numpy(on)
        assert torch.equal(_i32(t[:n, :K][on_t]), _i32(want.cpu()[on_t])) and (t[:n, K][on_t] == 1).all()
        assert (want.cpu()[on_t].sum(1) > 0.99).all()
        assert (t[:n][~on_t] == 0).all() and (t[n:] == -7.0).all()
        recycled_quiet += int((was_active & ~on).sum())
        was_active = on
        assert state.tolist()[NEXT] == n1
    assert recycled_quiet >= 2


# ---- refusals -------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments():
    """-2 from the host checks and nothing launched: every buffer keeps its fill."""
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib, ptr, stream
    jcap, K = 4, 3
    n = jcap * NF
    ring = torch.zeros(1, F_, 16, device="cuda")
    state = HF.live_state("cuda")
    state[AVAIL] = 100
    fs_d = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")
    power, floor = torch.full((n,), 2.0, device="cuda"), torch.full((n,), 1.0, device="cuda")
    active = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    sel = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    offs = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    cursor, count = HF.live_gate_state("cuda")
    table = torch.full((n, K + 1), 5.0, device="cuda")
    src = torch.zeros(B, K, device="cuda")
    out = torch.full((B, WIN[0], WIN[1], 8), 3.0, device="cuda", dtype=torch.bfloat16)
    lab = torch.full((B, 2), -5, dtype=torch.int64, device="cuda")
    live = {"ring": ptr(ring), "state": ptr(state), "fs": ptr(fs_d), "C": 1, "F": F_, "R": 16, "nf": NF, "st": ST,
            "Wf": 5, "Wt": 7, "Jcap": jcap, "n0": 0, "n1": 2 * NF}
    pw = dict(live, power=ptr(power))
    fl = dict(live, power=ptr(power), floor=ptr(floor), history=3, warmup=2)
    se = dict(live, power=ptr(power), floor=ptr(floor), active=ptr(active), sel=ptr(sel), cap=n, count=ptr(count),
              cursor=ptr(cursor), ratio=2.0, table=ptr(table), nrows=n, pitch=K + 1, offs=ptr(offs), noffs=4)
    ga = dict(live, B=B, taps=3, off=1, out=ptr(out), lab_out=ptr(lab), lab_w=2, sel=ptr(sel), cap=n,
              count=ptr(count), cursor=ptr(cursor))
    pr = {"state": ptr(state), "B": B, "nf": NF, "src": ptr(src), "softmax": 1, "K": K, "table": ptr(table),
          "nrows": n, "pitch": K + 1, "Jcap": jcap, "sel": ptr(sel), "cap": n, "count": ptr(count),
          "cursor": ptr(cursor)}
    # the same launchers without a selection, and the resident recording's two (3 x 2 windows of 5 x 7)
    none = dict(sel=0, count=0, cursor=0, cap=0)
    rec = torch.zeros(1, F_, 16, device="cuda")
    ts_d = torch.tensor([0, 9], dtype=torch.int32, device="cuda")
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    res = {"rec": ptr(rec), "fs": ptr(fs_d), "ts": ptr(ts_d), "C": 1, "F": F_, "T": 16, "nf": NF, "nt": 2, "B": B,
           "Wf": 5, "Wt": 7, "lo": 0, "hi": 2 * NF, "cursor": ptr(cursor), "sel": ptr(sel), "cap": n,
           "count": ptr(count)}
    wg = dict(res, taps=3, off=1, out=ptr(out), lab_out=ptr(lab), lab_w=2)
    wp = dict(res, src=ptr(src), softmax=1, K=K, probs=ptr(table), nprobs=n)
    bad = [
        (lib().ring_window_power, dict(pw, power=0)),
        (lib().ring_window_power, dict(pw, ring=0)),
        (lib().ring_window_power, dict(pw, state=0)),
        (lib().ring_window_power, dict(pw, fs=0)),
        (lib().ring_window_power, dict(pw, n0=1)),                 # not a whole time index
        (lib().ring_window_power, dict(pw, n1=(jcap + 1) * NF)),   # more indices than the ring has
        (lib().ring_window_power, dict(pw, n0=3 * NF)),            # n0 > n1
        (lib().running_floor, dict(fl, history=0)),
        (lib().running_floor, dict(fl, history=1025, warmup=1)),
        (lib().running_floor, dict(fl, warmup=4)),                 # warmup > history
        (lib().running_floor, dict(fl, warmup=0)),
        (lib().running_floor, dict(fl, history=4)),                # Jcap 4 < 3 + 2 indices
        (lib().running_floor, dict(fl, floor=0)),
        (lib().running_floor, dict(fl, power=0)),
        (lib().live_select, dict(se, cap=2 * NF - 1)),             # cap < n1 - n0
        (lib().live_select, dict(se, sel=0)),
        (lib().live_select, dict(se, count=0)),
        (lib().live_select, dict(se, cursor=0)),
        (lib().live_select, dict(se, table=0)),
        (lib().live_select, dict(se, active=0)),
        (lib().live_select, dict(se, offs=0)),
        (lib().live_select, dict(se, noffs=0)),
        (lib().live_select, dict(se, nrows=n - 1)),
        (lib().live_select, dict(se, pitch=0)),
        (lib().gather_windows_ring, dict(ga, sel=0)),
        (lib().gather_windows_ring, dict(ga, count=0)),
        (lib().gather_windows_ring, dict(ga, cursor=0)),
        (lib().gather_windows_ring, dict(ga, out=0)),
        (lib().gather_windows_ring, dict(ga, R=7)),
        (lib().gather_windows_ring, dict(ga, **dict(none, sel=ptr(sel), cap=n))),   # each of the three alone
        (lib().gather_windows_ring, dict(ga, **dict(none, count=ptr(count)))),
        (lib().gather_windows_ring, dict(ga, **dict(none, cursor=ptr(cursor)))),
        (lib().live_probs, dict(pr, pitch=K)),                     # the gated table has K + 1 columns
        (lib().live_probs, dict(pr, pitch=K + 2)),
        (lib().live_probs, dict(pr, table=0)),
        (lib().live_probs, dict(pr, nrows=n - 1)),
        (lib().live_probs, dict(pr, sel=0)),
        (lib().live_probs, dict(pr, count=0)),
        (lib().live_probs, dict(pr, **none)),                      # no selection: the table has K columns
    ]
    for fn, d in ((lib().gather_windows, wg), (lib().window_probs, wp)):
        bad += [
            (fn, dict(d, count=0)),                                # sel without count
            (fn, dict(d, sel=0)),                                  # count without sel
            (fn, dict(d, idx=ptr(idx))),                           # a selection with idx set, beside the cursor
            (fn, dict(d, idx=ptr(idx), cursor=0)),                 # and in its place
            (fn, dict(d, cursor=0)),                               # a selection with a null cursor
        ]
    for fn, d in bad:
        with pytest.raises(RuntimeError, match="rc=-2"):
            fn(stream(), d)
    torch.cuda.synchronize()
    assert (power == 2.0).all() and (floor == 1.0).all() and (active == 9).all() and (sel == -1).all()
    assert (offs == -1).all() and (table == 5.0).all() and (out.float() == 3.0).all() and (lab == -5).all()
    assert state.tolist() == [0, 100, 0, -1, 0] and cursor.item() == 0 and count.item() == 0
    with pytest.raises(ValueError):  # the wrappers check what a pointer cannot show: a ring below jcap * nf entries
        HF.ring_window_power(ring, state, fs_d, ST, WIN, power[:n - 1], jcap, 0, NF)
    with pytest.raises(ValueError):
        HF.running_floor(power, floor, NF, jcap, 0, NF, 1025, 1)


# ---- end to end -----------------------------------------------------------------------------------------------
T_E2E, CHUNKS_E2E, BATCH, CELL = 690, (1, 249, 130, 77, 233), 32, (50, 50)
HISTORY, WARMUP = 4, 2
MODELS = ["MTL", "multi_classifier"]
_runs = {}


class _Recorder:
    """ops.functional with live_map's raw results kept (the gated map before its division)."""

    def __init__(self, HF):
        self._HF, self.raw = HF, []

    def __getattr__(self, name):
        return getattr(self._HF, name)

    def live_map(self, *a, **k):
        m = self._HF.live_map(*a, **k)
        self.raw.append(m.clone())
        return m


def _fixture():
    from mtl_das_pytorch_amd.inference import WINDOW, window_power_reference, window_starts
    if "fix" not in _runs:
        rec = G.fixture()[0][:, :T_E2E].copy()
        fs, ts = window_starts(230, WINDOW[0], G.STRIDE[0]), window_starts(T_E2E, WINDOW[1], G.STRIDE[1])
        assert len(fs) == 14 and len(ts) == 10
        _runs["fix"] = (rec, fs, ts, window_power_reference(rec, fs, ts, WINDOW).reshape(14, 10).T.copy())
    return _runs["fix"]


def _e2e(model_type):
    """One model on the fixture: the gated offline result, and the live runs -- ungated, fixed floor with the map,
    running floor, the gate that keeps everything -- each with its replays per call and captures per call."""
    if model_type in _runs:
        return _runs[model_type]
    from mtl_das_pytorch_amd.inference import LiveRecording, predict_recording
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(1)
    m = build_model(model_type)
    m.train()  # non-trivial BN running statistics
    with torch.no_grad():
        m(torch.randn(8, 1, 100, 250))
    m.eval()
    rec = torch.from_numpy(_fixture()[0])

    def live(cell=None, **gate):
        lv = LiveRecording(m, model_type, 230, stride=G.STRIDE, cell=cell, ring=512, batch=BATCH, device="cuda",
                           use_engine=True, floor_history=HISTORY, floor_warmup=WARMUP, **gate)
        steps, step = [0], lv.backend.runner.live_step

        def counted():
            steps[0] += 1
            step()

        lv.backend.runner.live_step = counted
        lv.backend.HF = rec_hf = _Recorder(lv.backend.HF)
        outs, replays, caps, at = [], [], [], 0
        for i, n in enumerate(CHUNKS_E2E):  # every chunk is one piece: 512 - 250 = 262 samples at most
            chunk = rec[:, at:at + n]
            steps[0] = 0
            outs.append(lv.push(chunk.cuda() if i % 2 else chunk))  # device and host chunks
            replays.append(steps[0])
            caps.append(lv.captures)
            at += n
        steps[0] = 0
        outs.append(lv.flush())
        replays.append(steps[0])
        caps.append(lv.captures)
        state = lv.backend.state.tolist()
        lv.close()
        assert caps == [1] * len(caps) and state[:3] == [T_E2E, 140, 140]
        return outs, replays, rec_hf.raw

    r = {"off": predict_recording(m, model_type, rec, stride=G.STRIDE, batch=BATCH, device="cuda", use_engine=True,
                                  gate_db=G.GATE_DB, noise_floor=1.0),
         "plain": live(), "fixed": live(cell=CELL, gate_db=G.GATE_DB, noise_floor=1.0),
         "running": live(gate_db=G.GATE_DB, noise_floor="running"), "keep": live(gate_db=-100.0, noise_floor=1.0)}
    _runs[model_type] = r
    return r


def _cat(outs, k):
    return np.concatenate([o[k] for o in outs])


def _replays(outs, key=None):
    return [-(-int(o[key].sum() if key else len(o["positions"])) // BATCH) for o in outs]


@pytest.mark.parametrize("model_type", MODELS)
def test_live_fixed_floor_matches_gated_predict_recording(model_type):
    r = _e2e(model_type)
    off, (outs, replays, _) = r["off"], r["fixed"]
    want = ~(_fixture()[3] < 10.0 ** (G.GATE_DB / 10.0))  # [j][a]: the fp64 flags at a floor of 1
    assert want.sum() == 60
    pos = _cat(outs, "positions")
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    assert np.array_equal(pos[order], off["positions"])
    assert set(outs[-1]) == set(off) | {"floor_db", "map_columns"}
    active = _cat(outs, "active")
    assert np.array_equal(active, want.reshape(-1)) and np.array_equal(active[order], off["active"])
    assert np.array_equal(_cat(outs, "power_db")[order], off["power_db"])  # the same fp32 bits, the same log
    assert (_cat(outs, "floor_db") == 0).all()
    for k in [k for k in off if k.endswith("_pred")]:
        got = _cat(outs, k)
        assert np.array_equal(got[order], off[k]) and (got[~active] == -1).all() and (got[active] >= 0).all(), k
    for k in [k for k in off if k.endswith("_prob")]:
        got = _cat(outs, k)
        diff = np.abs(got[order].astype(np.float64) - off[k]).max()
        print(f"{model_type} gated live vs gated offline {k}: max abs diff {diff:.3e}")
        assert np.array_equal(got[order], off[k]), (k, diff)  # bit for bit: a row does not depend on its batch
        assert (got[~active] == 0).all()
    # one replay per 32 active windows of a piece, fewer than the ungated run's
    assert replays == _replays(outs, "active") and r["plain"][1] == _replays(r["plain"][0])
    print(f"{model_type} replays: gated {replays}, ungated {r['plain'][1]}")
    assert sum(replays) < sum(r["plain"][1])


@pytest.mark.parametrize("model_type", MODELS)
def test_live_running_floor_matches_the_reference(model_type):
    from mtl_das_pytorch_amd.inference import live_active_reference, running_floor_reference
    r = _e2e(model_type)
    (outs, replays, _), plain = r["running"], r["plain"][0]
    power = _fixture()[3]
    floor = running_floor_reference(power.reshape(-1), 14, HISTORY, WARMUP)
    want = live_active_reference(power, floor, G.GATE_DB)
    assert want.sum() == 46 and want.sum(1).tolist() == [14, 0, 0, 0, 0, 10, 12, 10, 0, 0]
    active = _cat(outs, "active")
    assert np.array_equal(active, want.reshape(-1))
    assert np.array_equal(_cat(outs, "positions"), _cat(plain, "positions"))
    fdb = _cat(outs, "floor_db")
    assert np.isneginf(fdb[:14]).all() and np.abs(fdb[14:] - 10 * np.log10(floor.reshape(-1)[14:])).max() < 1e-5
    assert np.abs(_cat(outs, "power_db") - 10 * np.log10(power.reshape(-1))).max() < 1e-5  # 2^-23 relative: 5e-7 dB
    for k in [k for k in plain[0] if k.endswith("_prob")]:
        got, ungated = _cat(outs, k), _cat(plain, k)
        assert np.array_equal(got[active], ungated[active]), k  # the ungated live run's bits
        assert (got[~active] == 0).all()
    for k in [k for k in plain[0] if k.endswith("_pred")]:
        got = _cat(outs, k)
        assert np.array_equal(got[active], _cat(plain, k)[active]) and (got[~active] == -1).all(), k
    assert replays == _replays(outs, "active") and sum(replays) < sum(r["plain"][1])


@pytest.mark.parametrize("model_type", MODELS)
def test_live_gate_that_keeps_everything_changes_nothing(model_type):
    r = _e2e(model_type)
    (outs, replays, _), (plain, plain_replays, _) = r["keep"], r["plain"]
    assert _cat(outs, "active").all() and replays == plain_replays
    for o, p in zip(outs, plain):
        assert set(o) == set(p) | {"active", "power_db", "floor_db"}
        for k in p:
            assert np.array_equal(o[k], p[k]), k


@pytest.mark.parametrize("model_type", MODELS)
def test_live_gated_map_matches_prediction_map(model_type):
    """The columns' NaN pattern is prediction_map(active=...)'s exactly.  Before the division, numerator and activity
    are within docs/ACCURACY.md's bound for live_map, (n + 3) * 2^-24 per cell, n the (fiber, time) window pairs
    covering it, against the fp64 map of the run's own rows."""
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map, window_map_reference
    r = _e2e(model_type)
    off, (outs, _, raw) = r["off"], r["fixed"]
    _, fs, ts, _ = _fixture()
    shape = (230, T_E2E)
    want = prediction_map(off, fs, ts, shape, CELL)
    firsts = [o["map_columns"]["first"] for o in outs] + [outs[-1]["map_columns"]["last"]]
    assert firsts[0] == 0 and firsts[-1] == 14 and firsts == sorted(firsts)
    for k in ("event_map", "distance_map", "distance_mean_m", "activity_map"):
        got = np.concatenate([o["map_columns"][k] for o in outs], -1)
        assert got.shape == want[k].shape and np.array_equal(np.isnan(got), np.isnan(want[k])), k
    empty = want["activity_map"] == 0
    assert empty.any() and not empty.all() and np.isnan(want["event_map"][:, empty]).all()
    # the undivided K + 1 class map the kernel wrote
    keys = [k for k in off if k.endswith("_prob")]
    table = np.concatenate([off[k] for k in keys] + [off["active"][:, None].astype(np.float32)], 1)  # quiet rows: 0
    ref = window_map_reference(table, fs, ts, shape, CELL)
    got = np.concatenate([m.cpu().numpy().astype(np.float64) for m in raw], -1)

    def count(starts, win, length, c):
        return np.array([sum(1 for s in starts if s < min(x + c, length) and s + win > x) for x in range(0, length, c)])
    pairs = count(fs, WINDOW[0], 230, CELL[0])[:, None] * count(ts, WINDOW[1], T_E2E, CELL[1])[None]
    bound = (pairs + 3) * 2.0 ** -24
    err = np.abs(got - ref)
    print(f"{model_type} gated live map: numerator worst abs err {err[:-1].max():.3e}, activity {err[-1].max():.3e}, "
          f"bound {bound.min():.3e} .. {bound.max():.3e}")
    assert got.shape == ref.shape and (err <= bound[None]).all(), err.max()
    ev = np.concatenate([o["map_columns"]["event_map"] for o in outs], -1)
    assert np.abs(ev[:, ~empty].sum(0) - 1).max() < 1e-4  # only active windows speak, and they sum to 1
