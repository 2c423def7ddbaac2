"""CPU: live inference on a growing recording -- the host's window / column bookkeeping against brute force, the time
weights against the whole-recording weights, and the torch backend of LiveRecording against predict_recording and
prediction_map on the concatenated chunks."""
import numpy as np
import pytest
import torch

WT, R = 7, 16
# sizes 1, R - Wt = 9 and 20 > R (split by push); totals 70 (T - Wt = 63: a multiple of every stride), 41 and 6 < Wt
SEQUENCES = [[1, 9, 20, 5, 35], [2, 9, 17, 1, 11, 1], [1, 2, 3], [7], [20, 1]]


@pytest.mark.parametrize("st", [1, 3, 7, 9])
@pytest.mark.parametrize("ct", [1, 2, 7, 10])
@pytest.mark.parametrize("chunks", SEQUENCES, ids=lambda c: "-".join(map(str, c)))
def test_bookkeeping_matches_brute_force(st, ct, chunks):
    from mtl_das_pytorch_amd.inference import LiveBook, window_starts
    book = LiveBook(WT, st, R, ct)
    seen_j, seen_q, total = [], [], 0
    for n in chunks:
        parts = book.split(n)
        assert sum(parts) == n and max(parts) <= R - WT and (n <= R - WT or len(parts) > 1)
        book.check_push(n)
        assert (book.total, book.j_done, book.q_done) == (total, len(seen_j), len(seen_q))  # a dry run
        for m in parts:
            (j0, j1), (q0, q1) = book.advance(m)
            seen_j += [(j, book.time_start(j)) for j in range(j0, j1)]
            seen_q += list(range(q0, q1))
        total += n
        assert book.total == total
        assert [j for j, _ in seen_j] == [j for j in range(total + 1) if j * st + WT <= total]
        assert all(t0 == j * st for j, t0 in seen_j)
        assert seen_q == [q for q in range(total + 1) if (q + 1) * ct <= total - WT]
    (j0, j1), (q0, q1) = book.finish()
    seen_j += [(j, book.time_start(j)) for j in range(j0, j1)]
    seen_q += list(range(q0, q1))
    T = total
    if T < WT:
        assert seen_j == [] and seen_q == []
    else:
        assert [t0 for _, t0 in seen_j] == list(window_starts(T, WT, st))
        assert [j for j, _ in seen_j] == list(range(len(seen_j)))  # each window once, in number order
        assert seen_q == list(range(-(-T // ct)))  # each column once
        if (T - WT) % st == 0:
            assert j1 == j0  # no extra window
    with pytest.raises(RuntimeError):
        book.advance(1)


@pytest.mark.parametrize("st", [1, 3, 7])
@pytest.mark.parametrize("ct", [1, 2, 7, 10])
@pytest.mark.parametrize("T", [7, 23, 41, 70])
def test_time_weights_match_the_whole_recording(st, ct, T):
    """A column's weights, taken while the stream runs (once it is final) or at its end, are those of
    window_cell_weights on the finished recording's start table."""
    from mtl_das_pytorch_amd.inference import live_time_weights, window_starts
    from mtl_das_pytorch_amd.ops.functional import window_cell_weights
    ts = window_starts(T, WT, st)
    want = window_cell_weights(ts, WT, T, ct)  # [nt, ncol]
    for q in range(want.shape[1]):
        forms = [T]
        # final at some total <= T: no knowledge of the end
        if (q + 1) * ct <= T - WT:
            forms.append(None)
        for end in forms:
            jlo, w = live_time_weights(q, ct, WT, st, end)
            full = np.zeros(len(ts))
            full[jlo:jlo + len(w)] = w
            assert jlo + len(w) <= len(ts)
            assert np.abs(full - want[:, q]).max() <= 1e-12, (q, end)
            assert abs(w.sum() - 1) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
F_, T_, STRIDE, CHUNKS, CELL = 200, 900, (100, 125), (1, 249, 130, 77, 443), (50, 125)
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
    """One offline and one live run (with the map) of Model A on the CPU, shared by the tests below."""
    from mtl_das_pytorch_amd.inference import LiveRecording, predict_recording
    if "runs" not in _cache:
        rec = torch.randn(F_, T_, generator=torch.Generator().manual_seed(3))
        off = predict_recording(_model(), "MTL", rec, stride=STRIDE, batch=8, use_engine=False)
        live = LiveRecording(_model(), "MTL", F_, stride=STRIDE, cell=CELL, ring=512, batch=8, use_engine=False)
        outs, at = [], 0
        for n in CHUNKS:
            outs.append(live.push(rec[:, at:at + n]))
            at += n
        assert at == T_ and live.total == T_
        outs.append(live.flush())
        live.close()
        _cache["runs"] = (rec, off, outs)
    return _cache["runs"]


def test_torch_live_matches_predict_recording():
    rec, off, outs = _runs()
    pos = np.concatenate([o["positions"] for o in outs])
    assert len(pos) == len(off["positions"]) == 14
    assert len(outs[0]["positions"]) == 0 and len(outs[1]["positions"]) == 2  # 1 sample; 250: the first index
    assert len(outs[-1]["positions"]) == 2 and (outs[-1]["positions"][:, 1] == 650).all()  # the end-aligned index
    order = np.lexsort((pos[:, 1], pos[:, 0]))
    order_off = np.lexsort((off["positions"][:, 1], off["positions"][:, 0]))
    assert np.array_equal(pos[order], off["positions"][order_off])
    for k in ("distance_prob", "event_prob"):
        got = np.concatenate([o[k] for o in outs])[order]
        err = np.abs(got.astype(np.float64) - off[k][order_off]).max()
        print(f"torch live vs offline {k}: max abs diff {err:.3e}")
        assert err <= 1e-5, (k, err)
    for k in ("distance_pred", "event_pred"):
        got = np.concatenate([o[k] for o in outs])
        prob = np.concatenate([o[k[:-4] + "prob"] for o in outs])
        assert np.array_equal(got, prob.argmax(1))


def test_torch_live_map_columns_match_prediction_map():
    from mtl_das_pytorch_amd.inference import WINDOW, prediction_map, window_starts
    rec, off, outs = _runs()
    fs, ts = window_starts(F_, WINDOW[0], STRIDE[0]), window_starts(T_, WINDOW[1], STRIDE[1])
    want = prediction_map(off, fs, ts, (F_, T_), CELL)
    at = 0
    for o in outs:  # each column once, in order
        mc = o["map_columns"]
        assert mc["first"] == at and mc["last"] >= at
        assert mc["event_map"].shape == (2, 4, mc["last"] - at)
        at = mc["last"]
    assert at == want["event_map"].shape[2] == 8
    # final while the stream runs: (q + 1) * 125 <= total - 250
    assert [o["map_columns"]["last"] for o in outs] == [0, 0, 1, 1, 5, 8]
    for k in ("event_map", "distance_map", "distance_mean_m"):
        got = np.concatenate([o["map_columns"][k] for o in outs], -1)
        err = np.abs(got - want[k]).max()
        print(f"torch live map {k}: max abs diff {err:.3e}")
        assert got.shape == want[k].shape and err <= 1e-6, (k, err)


def test_errors():
    from mtl_das_pytorch_amd.inference import LiveRecording
    m = _model()
    live = LiveRecording(m, "MTL", F_, stride=STRIDE, ring=512, batch=8, use_engine=False)
    with pytest.raises(ValueError):
        live.push(torch.zeros(2, F_, 10))  # wrong C
    with pytest.raises(ValueError):
        live.push(torch.zeros(1, F_ + 1, 10))  # wrong F
    assert live.total == 0
    live.push(torch.zeros(F_, 10))
    assert len(live.flush()["positions"]) == 0  # T < Wt: empty
    with pytest.raises(RuntimeError):
        live.push(torch.zeros(F_, 10))
    with pytest.raises(ValueError):
        LiveRecording(m, "MTL", F_, stride=STRIDE, ring=250, use_engine=False)  # below Wt + 1
    # a table of 2 time indices: 500 samples make 3 (starts 0, 125, 250); nothing is written before the raise
    small = LiveRecording(m, "MTL", F_, stride=STRIDE, ring=1024, use_engine=False, table_indices=2)
    with pytest.raises(ValueError, match="table"):
        small.push(torch.zeros(F_, 500))
    assert small.total == 0

    class Ctx:
        enabled, world, rank, device = True, 2, 0, torch.device("cpu")
    with pytest.raises(ValueError, match="world"):
        LiveRecording(m, "MTL", F_, stride=STRIDE, use_engine=False, ctx=Ctx())
