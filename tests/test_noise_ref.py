"""The SNR noise definition (data/noise.py, numpy fp64): statistics, determinism, edge shapes, and its plumbing
through the plain-PyTorch backend, the trainer and the command line.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from mtl_das_pytorch_amd.data import noise as nz

H, W = 100, 250
CASES = [(seed, draw, row) for seed in (1, 0x9E3779B97F4A7C15, 2 ** 64 - 1) for draw in (0, 2 ** 32 + 3)
         for row in (0, 7, 2 ** 32 + 11)]


def test_philox_known_answers():
    """Random123's published Philox-4x32-10 known-answer vectors, on the package's copy."""
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32)
    keys = [0, 0xFFFFFFFFFFFFFFFF, (0x299F31D0 << 32) | 0xA4093822]
    want = [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    for i in range(3):
        assert nz.philox_np(ctr[i:i + 1], keys[i])[0].tolist() == want[i]


@pytest.mark.parametrize("seed,draw,row", CASES)
def test_gaussian_statistics(seed, draw, row):
    """18 (seed, draw, row) cases at 100 x 250: mean, variance, lag-1 correlation along h and w, correlation with
    the next draw and with the next row.  Bounds: 5 / sqrt(n) (5 sqrt(2 / n) on the variance), n = H W."""
    n = H * W
    g = nz.gaussian([row, row + 1], 1, H, W, seed, draw, nz.STREAM_TRAIN)
    a, nxt_row = g[0, 0], g[1, 0]
    nxt_draw = nz.gaussian([row], 1, H, W, seed, draw + 1, nz.STREAM_TRAIN)[0, 0]
    b = 5.0 / np.sqrt(n)
    assert abs(a.mean()) < b
    assert abs(a.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs((a[1:] * a[:-1]).mean()) < b
    assert abs((a[:, 1:] * a[:, :-1]).mean()) < b
    assert abs((a * nxt_draw).mean()) < b
    assert abs((a * nxt_row).mean()) < b


@pytest.mark.parametrize("snr_db", [20.0, 0.0, -5.0])
def test_measured_snr(snr_db):
    """The SNR holds in expectation: |measured - target| < 0.25 dB on a 100 x 250 plane (estimator sigma 0.039 dB)."""
    rng = np.random.default_rng(3)
    X = (100.0 * rng.standard_normal((3, 2, H, W)) + 40.0).astype(np.float32)
    for form in ({"snr_db": snr_db}, {"snr": (snr_db, snr_db)}):
        y = nz.add_noise(X, [0, 1, 2], 11, 4, **form)
        meas = 10.0 * np.log10(nz.sample_power(X) / ((y - X) ** 2).mean((2, 3)))
        print(form, meas)
        assert np.abs(meas - snr_db).max() < 0.25


def test_determinism_and_independence_of_shape_and_batch():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6, 2, 9, 13)).astype(np.float32)
    P = nz.sample_power(X)
    rows = [4, 1, 4, 0]
    a = nz.add_noise(X, rows, 5, 2, snr=(0.0, 20.0), power=P)
    assert np.array_equal(a, nz.add_noise(X, rows, 5, 2, snr=(0.0, 20.0), power=P))
    assert np.array_equal(a[0], a[2])  # a row that appears twice gets the same noise
    perm = [3, 0, 2, 1]
    assert np.array_equal(a[perm], nz.add_noise(X, [rows[i] for i in perm], 5, 2, snr=(0.0, 20.0), power=P))
    assert not np.array_equal(a, nz.add_noise(X, rows, 5, 3, snr=(0.0, 20.0), power=P))
    assert not np.array_equal(a, nz.add_noise(X, rows, 6, 2, snr=(0.0, 20.0), power=P))
    # element (h, w) does not change when H grows; streams differ
    g9 = nz.gaussian(rows, 2, 9, 13, 5, 2, nz.STREAM_EVAL)
    g20 = nz.gaussian(rows, 2, 20, 13, 5, 2, nz.STREAM_EVAL)
    assert np.array_equal(g9, g20[:, :, :9])
    assert not np.array_equal(g9, nz.gaussian(rows, 2, 9, 13, 5, 2, nz.STREAM_TRAIN))
    # the per-sample level: inside the range, shared by the channels, one level when lo == hi
    s = nz.sample_snr(rows, 0.0, 20.0, 5, 2)
    assert ((s > 0.0) & (s <= 20.0)).all() and s[0] == s[2] and len(set(s.tolist())) == 3
    assert np.array_equal(nz.sample_snr(rows, 7.0, 7.0, 5, 2), np.full(4, 7.0))
    noise = a - X[rows]
    ratio = (noise / nz.gaussian(rows, 2, 9, 13, 5, 2, nz.STREAM_TRAIN)) ** 2 / P[rows][:, :, None, None]
    assert np.allclose(ratio, (10.0 ** (-s / 10.0))[:, None, None, None], rtol=1e-9)


@pytest.mark.parametrize("hw", [(7, 10), (9, 13)])
def test_rows_of_the_last_quad(hw):
    """H not a multiple of 4: the rows of the last (partial) quad are defined, finite and distinct."""
    h, w = hw
    g = nz.gaussian([0, 3], 3, h, w, 1, 0, nz.STREAM_TRAIN)
    assert g.shape == (2, 3, h, w) and np.isfinite(g).all()
    last = g[:, :, 4 * (h // 4):]
    assert last.shape[2] == h % 4 and len(np.unique(last)) == last.size
    # quads run vertically: row 4q + i of column w is word i of the call with counter q * W + w
    r = nz.philox_np(np.array([[(h // 4) * w + 2, 1 | (nz.STREAM_TRAIN << 8), 3, 0]], np.uint32), 1)[0]
    m0 = np.sqrt(-2.0 * np.log(nz.u01(r[0])))
    assert g[1, 1, 4 * (h // 4), 2] == m0 * np.cos(2.0 * np.pi * nz.u01(r[1]))


def test_constant_plane_is_left_alone():
    X = np.full((2, 1, 7, 10), 3.5, np.float32)
    assert np.array_equal(nz.add_noise(X, [0, 1], 1, 0, snr_db=-5.0), X.astype(np.float64))


# ---- torch-backend plumbing on a tiny synthetic set ---------------------------------------------------------
class _Tiny(nn.Module):
    """A 2-class log-softmax model that records its inputs."""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(6 * 9, 2)
        self.seen = []

    def forward(self, x):
        self.seen.append(x.detach().clone())
        return torch.log_softmax(self.fc(x.flatten(1)), 1)


def _tiny_backend(**kw):
    from mtl_das_pytorch_amd.engine.backends import TorchBackend
    from mtl_das_pytorch_amd.parallel.dist import init_distributed
    g = torch.Generator().manual_seed(0)
    X = 30.0 * torch.randn(16, 1, 6, 9, generator=g) + 5.0
    lab = torch.stack([torch.arange(16) % 16, torch.arange(16) % 2], 1)
    torch.manual_seed(0)
    be = TorchBackend(_Tiny(), "single_event", X, lab, X, lab, init_distributed(), batch=4, lr=1e-3,
                      weight_decay=0.0, **kw)
    return be, X


def test_torch_backend_train_noise_draws_and_resume():
    be, X = _tiny_backend(noise_snr=(0.0, 20.0), noise_seed=9)
    idx = torch.tensor([3, 8, 3, 15])
    be.train_batch(idx)
    be.train_batch(idx)
    ref = [nz.add_noise(X.numpy(), idx.numpy(), 9, d, snr=(0.0, 20.0)).astype(np.float32) for d in range(3)]
    assert np.array_equal(be.model.seen[0].numpy(), ref[0])
    assert np.array_equal(be.model.seen[1].numpy(), ref[1])
    assert not np.array_equal(ref[0], ref[1])
    st = be.optimizer_state()
    assert st["noise_draw"] == 2
    be2, _ = _tiny_backend(noise_snr=(0.0, 20.0), noise_seed=9)
    be2.load_optimizer_state(st)
    be2.train_batch(idx)
    assert np.array_equal(be2.model.seen[0].numpy(), ref[2])  # continues at d + 2
    # noise off: the clean rows
    be3, _ = _tiny_backend()
    be3.train_batch(idx)
    assert torch.equal(be3.model.seen[0], X[idx]) and be3.optimizer_state()["noise_draw"] == 0


def test_torch_backend_eval_noise():
    be, X = _tiny_backend(noise_snr=(0.0, 20.0), noise_seed=9)
    idx = torch.tensor([1, 2, 5, 1])
    be.set_eval_noise(5.0)
    be.eval_batch(idx, 4)
    be.eval_batch(idx, 4)
    ref = nz.add_noise(X.numpy(), idx.numpy(), nz.EVAL_SEED, 0, snr_db=5.0).astype(np.float32)
    assert np.array_equal(be.model.seen[0].numpy(), ref) and torch.equal(be.model.seen[0], be.model.seen[1])
    assert be.noise_draw == 0  # evaluation leaves the training draw alone
    be.set_eval_noise(None)
    be.eval_batch(idx, 4)
    assert torch.equal(be.model.seen[2], X[idx])


def test_trainer_evaluate_at_snr(tmp_path):
    """evaluate(..., snr_db=S) twice gives identical metrics, differs from the clean pass' inputs only through the
    evaluation noise, leaves the training draw alone and returns the backend to the clean eval."""
    from mtl_das_pytorch_amd.engine.trainer import Trainer
    from mtl_das_pytorch_amd.utils.config import TrainConfig
    cfg = TrainConfig(model="single_event", synthetic=1, batch_size=8, epoch_num=0, val_every=1, GPU_device=False,
                      output_savedir=str(tmp_path), save_threshold=2.0, noise_snr_db=[0.0, 20.0], seed=3)
    tr = Trainer(cfg)
    tr.run()
    assert tr.backend.noise_snr == (0.0, 20.0) and tr.backend.noise_seed == 3
    X, lab = tr.val_src.X, tr.val_src.labels
    tr.backend.noise_draw = 5
    a = tr.evaluate(X, lab, snr_db=-5.0)
    b = tr.evaluate(X, lab, snr_db=-5.0)
    c = tr.evaluate(X, lab)
    assert a == b
    assert a["loss"] != c["loss"]
    assert tr.backend.noise_draw == 5 and tr.backend.eval_snr_db is None
    # the sweep scores the synthetic samples' clean signals (the set itself carries 6-20 dB noise)
    from mtl_das_pytorch_amd.engine.trainer import load_datasets
    clean = load_datasets(cfg, tr.device, synthetic_noise=False)[1]
    assert torch.equal(clean.labels, lab) and not torch.equal(clean.X, X)
    rows = tr.snr_sweep([20.0, -5.0])
    assert [r["snr_db"] for r in rows] == [20.0, -5.0]
    assert rows[1]["loss"] == tr.evaluate(clean.X, clean.labels, snr_db=-5.0)["loss"]
    import json
    import os
    with open(os.path.join(tr.save_dir, "snr_sweep.json")) as f:
        assert [r["snr_db"] for r in json.load(f)["levels"]] == [20.0, -5.0]
    tr.close()


# ---- command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_test", [False, True])
def test_cli_flags(is_test):
    from mtl_das_pytorch_amd.utils.config import build_parser, config_from_args
    ap = build_parser(is_test)
    c = config_from_args(ap.parse_args([]), is_test)
    assert c.noise_snr_db is None and c.snr_sweep == [] and c.noise_seed == c.seed
    c = config_from_args(ap.parse_args(["--noise_snr_db", "0,20", "--seed", "4", "--snr_sweep", "20,10,5,0,-5"]), is_test)
    assert c.noise_snr_db == [0.0, 20.0] and c.noise_seed == 4 and c.snr_sweep == [20.0, 10.0, 5.0, 0.0, -5.0]
    c = config_from_args(ap.parse_args(["--noise_snr_db", "-5", "--noise_seed", "77"]), is_test)
    assert c.noise_snr_db == [-5.0, -5.0] and c.noise_seed == 77
    with pytest.raises(ValueError):
        config_from_args(ap.parse_args(["--noise_snr_db", "20,0"]), is_test)
    with pytest.raises(ValueError, match="resident"):  # noise on the streaming ring: refused at start-up
        config_from_args(ap.parse_args(["--noise_snr_db", "0,20", "--dataset_ram", "False"]), is_test)
