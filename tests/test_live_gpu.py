"""GPU: live inference on a growing recording (csrc/live.hip) -- the ring append and ring gather against the linear
gather_windows on the linearised recording, live_probs against window_probs, live_map against the fp64 map of the
whole recording, and LiveRecording on the engine end to end against predict_recording.

Small geometry of the kernel tests: window 5 x 7, F = 9, fiber stride 2 (starts 0, 2, 4), time stride 3, batch 4,
chunks 1, 3, 9, 2, 8 = 23 samples, so the time starts are 0, 3, .., 15 and the end-aligned 16 ((23 - 7) mod 3 = 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, F_, SF, ST, B = (5, 7), 9, 2, 3, 4
CHUNKS = (1, 3, 9, 2, 8)
T_ = sum(CHUNKS)
TOTAL, AVAIL, NEXT, JEND, TEND = range(5)


def _bits(t):
    return t.view(torch.int16)


def _geometry():
    from mtl_das_pytorch_amd.inference import window_starts
    fs, ts = window_starts(F_, WIN[0], SF), window_starts(T_, WIN[1], ST)
    assert list(fs) == [0, 2, 4] and list(ts) == [0, 3, 6, 9, 12, 15, 16]
    return fs, ts


def _pieces(n, step):
    return [min(step, n - i) for i in range(0, n, step)]


@pytest.mark.parametrize("R", [16, 11])
@pytest.mark.parametrize("C,taps,off", [(1, 3, 1), (3, 0, 0)])
def test_ring_gather_matches_linear_gather(R, C, taps, off):
    """After every append, every window that became available is cut from the ring and compared bit for bit with
    gather_windows (idx form) on the whole linear recording; the ring starts as NaN, so a read of a column not yet
    written, or of a padding row, shows.  The output is followed by sentinels."""
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib, ptr, stream
    fs, ts = _geometry()
    nf, nt = len(fs), len(ts)
    full = torch.randn(C, F_, T_, generator=torch.Generator().manual_seed(7)).cuda()
    ring = torch.full((C, F_, R), float("nan"), device="cuda")
    state = HF.live_state("cuda")
    fs_d = torch.as_tensor(fs, dtype=torch.int32).cuda()
    M = B * WIN[0] * WIN[1] * 8
    with pytest.raises(ValueError):  # more than R - Wt samples at once: push splits, the kernel level refuses
        HF.ring_append(ring, state, full[:, :, :R - WIN[1] + 1].contiguous(), nf, ST, WIN[1])
    assert state.tolist() == [0, 0, 0, -1, 0] and torch.isnan(ring).all()

    done = [0]
    partial = straddle = 0

    def evaluate(avail, jend=None):
        nonlocal partial, straddle
        while done[0] < avail:
            nxt = done[0]
            state[NEXT] = nxt
            out = torch.full((M + 64,), 123.0, device="cuda", dtype=torch.bfloat16)
            lab = torch.full((B * 2 + 8,), -5, device="cuda", dtype=torch.int64)
            lib().gather_windows_ring(stream(), {
                "ring": ptr(ring), "state": ptr(state), "fs": ptr(fs_d), "C": C, "F": F_, "R": R, "nf": nf, "st": ST,
                "B": B, "Wf": WIN[0], "Wt": WIN[1], "taps": taps, "off": off, "out": ptr(out), "lab_out": ptr(lab),
                "lab_w": 2})
            rows = []
            for r in range(B):
                n = nxt + r
                if n < avail:
                    j, a = divmod(n, nf)
                    rows.append(a * nt + j)  # the offline table is fiber-major
                    t0 = int(ts[j])
                    straddle += int(t0 % R + WIN[1] > R)
                else:
                    rows.append(-1)
            partial += int(-1 in rows)
            ref, _ = HF.gather_windows(full, fs, ts, WIN, B, idx=torch.tensor(rows, device="cuda"), taps=taps, off=off)
            got = out[:M].view(B, WIN[0], WIN[1], 8)
            assert not torch.isnan(got.float()).any()
            assert torch.equal(_bits(got), _bits(ref)), (R, nxt)
            for r, n in enumerate(rows):
                if n < 0:
                    assert (_bits(got[r]) == 0).all()
            assert (out[M:].float() == 123.0).all() and (lab[:B * 2] == 0).all() and (lab[B * 2:] == -5).all()
            assert state.tolist()[NEXT] == nxt  # the gather reads the counter, live_probs advances it
            done[0] = min(avail, nxt + B)

    total = 0
    for n in CHUNKS:
        for m in _pieces(n, R - WIN[1]):
            HF.ring_append(ring, state, full[:, :, total:total + m].contiguous(), nf, ST, WIN[1])
            total += m
            avail = ((total - WIN[1]) // ST + 1) * nf if total >= WIN[1] else 0
            s = state.tolist()
            assert (s[TOTAL], s[AVAIL], s[JEND]) == (total, avail, -1)
            evaluate(avail)
    # the ring holds the last R samples where they belong
    cols = torch.arange(max(0, T_ - R), T_)
    assert torch.equal(ring[:, :, cols % R].cpu(), full[:, :, cols].cpu())
    HF.ring_append(ring, state, None, nf, ST, WIN[1], flush=True)
    s = state.tolist()
    assert (s[TOTAL], s[AVAIL], s[JEND], s[TEND]) == (T_, nt * nf, nt - 1, T_ - WIN[1])
    evaluate(nt * nf)
    assert done[0] == nt * nf and partial >= 2 and straddle >= 1


def test_launchers_refuse_bad_arguments():
    """-2 from the host checks, nothing launched: the huge batch never touches memory."""
    from mtl_das_pytorch_amd.ops import functional as HF
    from mtl_das_pytorch_amd.ops.hip import lib, ptr, stream
    ring = torch.zeros(1, F_, 16, device="cuda")
    ring3 = torch.zeros(3, F_, 16, device="cuda")
    state = HF.live_state("cuda")
    fs_d = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")
    chunk = torch.zeros(1, F_, 10, device="cuda")
    out = torch.zeros(B, WIN[0], WIN[1], 8, device="cuda", dtype=torch.bfloat16)
    lab = torch.zeros(B, 2, dtype=torch.int64, device="cuda")
    table = torch.zeros(5, 3, device="cuda")
    src = torch.zeros(B, 3, device="cuda")
    app = {"ring": ptr(ring), "state": ptr(state), "C": 1, "F": F_, "R": 16, "nf": 3, "st": ST, "Wt": 7,
           "chunk": ptr(chunk), "n": 9, "flush": 0}
    gat = {"ring": ptr(ring), "state": ptr(state), "fs": ptr(fs_d), "C": 1, "F": F_, "R": 16, "nf": 3, "st": ST,
           "B": B, "Wf": 5, "Wt": 7, "taps": 3, "off": 1, "out": ptr(out), "lab_out": ptr(lab), "lab_w": 2}
    prb = {"state": ptr(state), "B": B, "nf": 3, "src": ptr(src), "softmax": 1, "K": 3, "table": ptr(table),
           "nrows": 5, "Jcap": 2}
    bad = [
        (lib().ring_append, dict(app, n=10)),            # n > R - Wt
        (lib().ring_append, dict(app, R=7)),             # R < Wt + 1
        (lib().ring_append, dict(app, ring=0)),
        (lib().ring_append, dict(app, state=0)),
        (lib().ring_append, dict(app, chunk=0)),
        (lib().gather_windows_ring, dict(gat, R=7)),
        (lib().gather_windows_ring, dict(gat, fs=0)),
        (lib().gather_windows_ring, dict(gat, out=0)),
        (lib().gather_windows_ring, dict(gat, ring=ptr(ring3), C=3)),  # taps > 0 with C != 1
        (lib().gather_windows_ring, dict(gat, B=1 << 20, Wf=64, Wt=32, F=64, R=64)),  # B Wf Wt = 2^31
        (lib().live_probs, prb),                         # 5 rows < Jcap * nf = 6
        (lib().live_probs, dict(prb, nrows=6, table=0)),
    ]
    for fn, d in bad:
        with pytest.raises(RuntimeError, match="rc=-2"):
            fn(stream(), d)
    mp = {"table": ptr(table), "fs": ptr(fs_d), "map": ptr(out), "wf": ptr(src), "wt": ptr(src), "jlo": ptr(lab),
          "jn": ptr(fs_d), "mf": 4, "mw": 1, "K": 3, "F": F_, "Wf": 5, "cf": 2, "nfc": 5, "Jcap": 2, "nrows": 5}
    bad_maps = [
        (mp, [0, 2, 4]),                   # a table below Jcap * nf rows
        (dict(mp, nrows=6), [0, 2, 3]),    # fiber row 8 of F = 9 is in no window
        (dict(mp, nrows=6), [0, 4, 2]),    # starts not increasing
    ]
    for d, fs_h in bad_maps:
        with pytest.raises(RuntimeError, match="rc=-2"):
            lib().live_map(stream(), d, fs_h, [0], [1])
    with pytest.raises(ValueError):
        HF.gather_windows_ring(torch.zeros(1, F_, 7, device="cuda"), state, [0, 2, 4], ST, WIN, B)
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0, 0, -1, 0]


@pytest.mark.parametrize("form", ["softmax", "logp"])
def test_live_probs_matches_window_probs(form):
    """10 windows in batches of 4 into a table of Jcap = 2 time indices (it wraps: j = 0 .. 3): after every call the
    whole table is bit-equal to window_probs (idx form) writing the same rows, so padding rows and the two rows past
    Jcap * nf keep their sentinel; next advances by the valid count and stops at avail."""
    from mtl_das_pytorch_amd.ops import functional as HF
    nf, jcap, avail = 3, 2, 10
    g = torch.Generator().manual_seed(11)
    K = 5 if form == "softmax" else 18
    table = torch.full((jcap * nf + 2, K), -7.0, device="cuda")
    ref = table.clone()
    state = HF.live_state("cuda")
    state[AVAIL] = avail
    state[TOTAL] = 16
    nxt = 0
    for step in range(4):
        if form == "softmax":
            src, ncls = (8 * torch.randn(B, K, generator=g)).cuda(), None
        else:
            logp = torch.full((2, B, 16), -50.0)
            logp[0] = torch.log_softmax(3 * torch.randn(B, 16, generator=g), 1)
            logp[1, :, :2] = torch.log_softmax(3 * torch.randn(B, 2, generator=g), 1)
            src, ncls = logp.cuda(), [16, 2]
        rows = []
        for r in range(B):
            j, a = divmod(nxt + r, nf)
            rows.append((j % jcap) * nf + a if nxt + r < avail else -1)
        HF.live_probs(src, table, state, nf, jcap, ncls=ncls)
        HF.window_probs(src, ref, idx=torch.tensor(rows, device="cuda"), ncls=ncls)
        valid = sum(r >= 0 for r in rows)
        assert valid == (4, 4, 2, 0)[step]
        nxt += valid
        assert state.tolist() == [16, avail, nxt, -1, 0]
        assert torch.equal(table.view(torch.int32), ref.view(torch.int32)), step
        assert (table[jcap * nf:] == -7.0).all()
    assert nxt == avail and (table[:jcap * nf] >= 0).all()  # every row of the ring table was written (and rewritten)


def _pairs(fs, ts, shape, cell):
    """[nfc, ntc]: the (fiber window, time window) pairs that overlap each cell."""
    def count(starts, win, length, c):
        return np.array([sum(1 for s in starts if s < min(x + c, length) and s + win > x) for x in range(0, length, c)])
    return count(fs, WIN[0], shape[0], cell[0])[:, None] * count(ts, WIN[1], shape[1], cell[1])[None]


@pytest.mark.parametrize("cell", [(2, 2), (4, 5)])
def test_live_map_final_columns_match_fp64(cell):
    """The stream of the gather test with random probabilities: every column, computed when it becomes final from a
    ring table of 6 time indices (7 are written: it wraps), against window_map_reference of the whole recording's
    table.  Bound (n + 3) * 2^-24 absolute per cell, n = the (fiber, time) window pairs summed: the two weights, their
    product and its product with the probability round once each (4 * 2^-24 of a total that is at most 1, the
    weights being non-negative with sum 1 and the probabilities at most 1) and the n - 1 additions once each."""
    from mtl_das_pytorch_amd.inference import LiveBook, live_time_weights, window_map_reference
    from mtl_das_pytorch_amd.ops import functional as HF
    fs, ts = _geometry()
    nf, nt, K, jcap = len(fs), len(ts), 3, 6
    p = torch.rand(nt, nf, K, generator=torch.Generator().manual_seed(13))  # [j][a][k]
    want = window_map_reference(p.permute(1, 0, 2).reshape(nf * nt, K).numpy(), fs, ts, (F_, T_), cell, WIN)
    bound = (_pairs(fs, ts, (F_, T_), cell) + 3) * 2.0 ** -24
    table = torch.full((jcap * nf, K), float("nan"), device="cuda")
    book = LiveBook(WIN[1], ST, 16, cell[1], table_indices=jcap)
    got = np.full(want.shape, np.nan)
    emitted, recomputed, worst = [], 0, 0.0

    def step(js, qs, T):
        nonlocal recomputed, worst
        for j in range(*js):
            table[(j % jcap) * nf:(j % jcap + 1) * nf] = p[j].cuda()
        # columns emitted earlier whose rows are all still in the table: the same bits again
        for q, jlo, w, old in emitted:
            if jlo >= book.j_done - jcap:
                again = HF.live_map(table, fs, F_, WIN[0], cell[0], jcap, [jlo], [w])
                assert torch.equal(again[:, :, 0].cpu(), old)
                recomputed += 1
        if qs[1] > qs[0]:
            cols = [live_time_weights(q, cell[1], WIN[1], ST, T) for q in range(*qs)]
            m = HF.live_map(table, fs, F_, WIN[0], cell[0], jcap, [c[0] for c in cols], [c[1] for c in cols]).cpu()
            assert m.shape == (K, want.shape[1], qs[1] - qs[0])
            for i, q in enumerate(range(*qs)):
                assert np.isnan(got[:, :, q]).all()  # emitted once
                got[:, :, q] = m[:, :, i].numpy()
                emitted.append((q, cols[i][0], cols[i][1], m[:, :, i].clone()))

    for n in CHUNKS:
        for m in book.split(n):
            js, qs = book.advance(m)
            step(js, qs, None)
    js, qs = book.finish()
    assert js == (nt - 1, nt)
    step(js, qs, T_)
    err = np.abs(got - want)
    assert not np.isnan(got).any()
    print(f"live_map cell {cell}: worst abs err {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
    assert (err <= bound[None]).all(), (err.max(), bound.max())
    assert recomputed >= 1


# ---------------------------------------------------------------------------------------------------------------
E2E_F, E2E_T, E2E_STRIDE, E2E_CHUNKS, E2E_CELL = 200, 900, (100, 125), (1, 249, 130, 77, 443), (50, 125)


@pytest.mark.parametrize("model_type", ["MTL", "multi_classifier"])
def test_live_recording_engine_matches_predict_recording(model_type):
    """The same windows as predict_recording(use_engine=True), bit-equal probabilities: on the offline path 14 windows
    evaluated in three batch orders, with and without padding rows, gave bit-equal tables for both models
    (docs/ACCURACY.md, Live inference), so the position of a window in its batch may not show.  One capture for the
    whole stream; the map columns against the fp64 map of the live run's own probabilities."""
    from mtl_das_pytorch_amd.inference import (WINDOW, LiveRecording, _task_maps, predict_recording,
                                               window_map_reference, window_starts)
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(1)
    m = build_model(model_type)
    m.train()  # non-trivial BN running statistics, so eval mode is exercised
    with torch.no_grad():
        m(torch.randn(8, 1, 100, 250))
    m.eval()
    rec = torch.randn(E2E_F, E2E_T, generator=torch.Generator().manual_seed(3))
    off = predict_recording(m, model_type, rec, stride=E2E_STRIDE, batch=8, device="cuda", use_engine=True)
    live = LiveRecording(m, model_type, E2E_F, stride=E2E_STRIDE, cell=E2E_CELL, ring=512, batch=8, device="cuda",
                         use_engine=True)
    outs, at, caps = [], 0, []
    for i, n in enumerate(E2E_CHUNKS):
        chunk = rec[:, at:at + n]
        outs.append(live.push(chunk.cuda() if i % 2 else chunk))  # device and host chunks
        caps.append(live.captures)
        at += n
    outs.append(live.flush())
    caps.append(live.captures)
    state = live.backend.state.tolist()
    live.close()
    assert caps == [1] * len(caps), caps  # captured once, before the first window; no push re-captures
    assert state[:3] == [E2E_T, 14, 14]

    pos = np.concatenate([o["positions"] for o in outs])
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    assert len(pos) == 14 and np.array_equal(pos[order], off["positions"])  # the offline table is sorted already
    keys = [k for k in off if k.endswith("_prob")]
    assert keys and set(off) <= set(outs[-1])
    for k in keys:
        got = np.concatenate([o[k] for o in outs])[order]
        diff = np.abs(got.astype(np.float64) - off[k]).max()
        print(f"{model_type} live vs offline {k}: max abs diff {diff:.3e}")
        assert np.array_equal(got, off[k]), (k, diff)
    for k in [k for k in off if k.endswith("_pred")]:
        assert np.array_equal(np.concatenate([o[k] for o in outs])[order], off[k]), k

    fs, ts = window_starts(E2E_F, WINDOW[0], E2E_STRIDE[0]), window_starts(E2E_T, WINDOW[1], E2E_STRIDE[1])
    table = np.concatenate([np.concatenate([o[k] for o in outs])[order] for k in keys], 1)
    want = window_map_reference(table, fs, ts, (E2E_F, E2E_T), E2E_CELL)
    firsts = [o["map_columns"]["first"] for o in outs] + [outs[-1]["map_columns"]["last"]]
    assert firsts == [0, 0, 0, 1, 1, 5, 8]  # (q + 1) * 125 <= total - 250; flush: the rest
    got = np.concatenate([o["map_columns"]["class_map"] for o in outs], -1)

    def count(starts, win, length, c):
        return np.array([sum(1 for s in starts if s < min(x + c, length) and s + win > x) for x in range(0, length, c)])
    pairs = count(fs, WINDOW[0], E2E_F, E2E_CELL[0])[:, None] * count(ts, WINDOW[1], E2E_T, E2E_CELL[1])[None]
    bound = (pairs + 3) * 2.0 ** -24
    err = np.abs(got - want)
    print(f"{model_type} live class map: worst abs err {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
    assert got.shape == want.shape and (err <= bound[None]).all(), err.max()
    # the task maps are sums of class maps (Model C: 16 joint classes per event type, 2 per distance bin)
    tm = _task_maps(want)
    per = {"event_map": 16, "distance_map": 2} if model_type == "multi_classifier" else {"event_map": 1, "distance_map": 1}
    for k, nsum in per.items():
        g = np.concatenate([o["map_columns"][k] for o in outs], -1)
        assert g.shape == tm[k].shape and (np.abs(g - tm[k]) <= nsum * bound[None]).all(), k
    assert np.concatenate([o["map_columns"]["distance_mean_m"] for o in outs], -1).shape == (4, 8)
