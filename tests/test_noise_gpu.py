"""GPU, kernel level: the SNR noise of the batch gather (csrc/augment.hip) against its numpy fp64 definition
(data/noise.py).

Shapes are the smallest that can go wrong: 5 dataset rows, a batch of 3 with a repeated row, 7 x 10 and 9 x 13 images
(H not a multiple of the vertical Philox quad), the packed stems (taps, off) = (3, 1) and (7, 3) and 1-3 unpacked
channels, index and schedule form; one case at the models' 100 x 250 with B = 32 and 7 taps.  Everything the kernel may
not read is NaN-poisoned and the outputs are followed by sentinels.
"""
import numpy as np
import pytest
import torch

from mtl_das_pytorch_amd.data import noise as nz

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567891  # above 2^63: both key words in use
DRAW = 2 ** 32 + 3        # the counter holds draw mod 2^32
SENT = 12288.0  # (exact in bf16)
FORMS = [("pack", 3, 1), ("pack", 7, 3), ("chan", 1, 0), ("chan", 2, 0), ("chan", 3, 0)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def layout(v: torch.Tensor, taps: int, off: int) -> torch.Tensor:
    """[B, Cin, H, W] -> the stem's [B, H, W, 8] input: channels zero-padded to 8, or (taps > 0) channel j of pixel
    (h, w) = v[h - off + j][w], zero outside the image."""
    B, C, H, W = v.shape
    out = torch.zeros(B, H, W, 8, dtype=v.dtype)
    if taps == 0:
        out[..., :C] = v.permute(0, 2, 3, 1)
        return out
    for j in range(taps):
        lo, hi = max(0, off - j), min(H, H + off - j)  # pixels h with 0 <= h - off + j < H
        out[:, lo:hi, :, j] = v[:, 0, lo - off + j:hi - off + j, :]
    return out


class Case:
    """One launch of gather_batch_noise with the test hook, and its inputs."""

    def __init__(self, H, W, Cin, taps, off, sched, N=5, rows=(4, 1, 4), snr=(10.0, 10.0), stream=0, draw=DRAW,
                 seed=SEED, X=None):
        from mtl_das_pytorch_amd.ops import functional as F
        g = torch.Generator().manual_seed(H * 1000 + W * 10 + Cin)
        self.Xc = (100.0 * torch.randn(N, Cin, H, W, generator=g) + 30.0) if X is None else X  # scaled, not centred
        self.rows = list(rows)
        B = len(rows)
        unused = [r for r in range(N) if r not in rows]
        self.P = F.sample_power(self.Xc.cuda())
        Xp, Pp = self.Xc.clone(), self.P.clone()
        Xp[unused] = float("nan")  # rows the launch may not read
        Pp[unused] = float("nan")
        lab = torch.arange(2 * N).view(N, 2) + 100
        lab[unused] = -777
        if sched:  # [nrows = 2][B] schedule with cursor 3: row 3 mod 2 = 1; row 0 points at the poisoned rows
            other = (unused * B)[:B] if unused else self.rows
            idx = torch.tensor([other, self.rows]).cuda()
            cursor = torch.tensor([3]).cuda()
        else:
            idx, cursor = torch.tensor(self.rows).cuda(), None
        n_out = B * H * W * 8
        self.out = torch.full((n_out + 64,), SENT, dtype=torch.bfloat16, device="cuda")
        self.dbg = torch.full((B * Cin * H * W + 16,), SENT, device="cuda")
        self.zero = torch.full((40,), 7.0, device="cuda")
        self.snr = torch.tensor(snr, dtype=torch.float32).cuda()
        self.draw = torch.tensor([draw]).cuda()
        _, self.lab = F.gather_batch_noise(Xp.cuda(), lab.cuda(), idx, Pp, self.snr, self.draw, seed,
                                           noise_stream=stream, taps=taps, off=off, zero=[self.zero[4:36]],
                                           cursor=cursor, out=self.out, dbg=self.dbg)
        torch.cuda.synchronize()
        self.shape = (B, Cin, H, W)
        self.taps, self.off, self.seed, self.d, self.stream, self.snr_host = taps, off, seed, draw, stream, snr
        self.want_lab = lab[self.rows]
        self.y = self.dbg[:B * Cin * H * W].view(B, Cin, H, W).cpu()
        self.o = self.out[:n_out].view(B, H, W, 8).cpu()

    def reference(self):
        """(y, x, sigma, g) in fp64 from the definition, with the device power table the launch read."""
        B, Cin, H, W = self.shape
        x = self.Xc[self.rows].double().numpy()
        P = self.P.double().cpu().numpy()[self.rows]
        lo, hi = self.snr_host
        level = nz.sample_snr(self.rows, lo, hi, self.seed, self.d)
        sig = nz.sigma(P, level)[:, :, None, None]
        g = nz.gaussian(self.rows, Cin, H, W, self.seed, self.d, self.stream)
        return x + sig * g, x, sig, g

    def check(self):
        B, Cin, H, W = self.shape
        y, x, sig, g = self.reference()
        # the unrounded values against fp64: fp32 logf, sincosf and one multiply-add
        scale = np.abs(x) + sig * (1.0 + np.abs(g))
        ratio = float((np.abs(self.y.double().numpy() - y) / scale).max())
        print(f"dbg worst |err| / (|x| + sigma (1 + |g|)) = {ratio:.3e}  [{H}x{W} Cin {Cin} taps {self.taps}]")
        assert ratio <= 1e-5
        # the stored bf16: round-to-nearest-even of the kernel's own fp32 values, in the stem's layout
        want = layout(self.y, self.taps, self.off).to(torch.bfloat16)
        assert torch.equal(_bits(self.o), _bits(want))
        real = self.taps or Cin
        assert (_bits(self.o[..., real:]) == 0).all()  # padding channels: exactly 0
        if self.taps:  # out-of-image taps: exactly 0
            assert (_bits(self.o[:, 0, :, :self.off]) == 0).all()
            assert (_bits(self.o[:, H - 1, :, self.off + 1:]) == 0).all()
        assert torch.equal(self.lab.cpu(), self.want_lab)
        z = self.zero.cpu()
        assert (z[4:36] == 0).all() and (z[:4] == 7).all() and (z[36:] == 7).all()
        assert (self.out[B * H * W * 8:].float() == SENT).all() and (self.dbg[B * Cin * H * W:] == SENT).all()
        for i, r in enumerate(self.rows):  # a repeated row gets identical noise in both batch positions
            j = self.rows.index(r)
            if j != i:
                assert torch.equal(self.y[i], self.y[j]) and torch.equal(_bits(self.o[i]), _bits(self.o[j]))
        return ratio


def test_sample_power_against_fp64():
    from mtl_das_pytorch_amd.ops import functional as F
    g = torch.Generator().manual_seed(1)
    for H, W in ((7, 10), (9, 13), (100, 250)):
        X = 100.0 * torch.randn(5, 3, H, W, generator=g) + 30.0
        X[1, 0] = torch.randn(H, W, generator=g) + 1e4  # mean 1e4, unit variance: a one-pass fp32 form fails
        X[2, 1] = -3.25                                  # constant planes: exactly 0
        X[3, 2] = 1e4
        P = F.sample_power(X.cuda()).double().cpu().numpy()
        ref = nz.sample_power(X.numpy())
        assert P[2, 1] == 0.0 and P[3, 2] == 0.0
        ok = ref > 0
        err = np.abs(P[ok] - ref[ok]) / ref[ok]
        print(f"sample_power {H}x{W}: worst relative error {err.max():.3e}")
        assert err.max() <= 1e-5
        x32 = X[1, 0].float()
        one_pass = float((x32 * x32).sum() / (H * W) - (x32.sum() / (H * W)) ** 2)
        print(f"  (one-pass fp32 on the mean-1e4 plane: {one_pass:.4f} vs {ref[1, 0]:.4f})")


@pytest.mark.parametrize("sched", [False, True], ids=["index", "schedule"])
@pytest.mark.parametrize("form", FORMS, ids=[f"{k}{a}_{b}" for k, a, b in FORMS])
@pytest.mark.parametrize("hw", [(7, 10), (9, 13)], ids=["7x10", "9x13"])
def test_noise_gather_small(hw, form, sched):
    kind, a, b = form
    Cin, taps, off = (1, a, b) if kind == "pack" else (a, 0, 0)
    Case(hw[0], hw[1], Cin, taps, off, sched).check()


def test_noise_gather_model_shape():
    """100 x 250, B = 32, 7 taps (Model A's stem), 40 dataset rows with repeats, a per-sample level."""
    rows = torch.randint(0, 40, (32,), generator=torch.Generator().manual_seed(2)).tolist()
    rows[5] = rows[20]
    Case(100, 250, 1, 7, 3, True, N=40, rows=rows, snr=(0.0, 20.0)).check()


@pytest.mark.parametrize("form", [("pack", 7, 3), ("chan", 3, 0)], ids=["pack7_3", "chan3"])
def test_zero_power_equals_clean_gather(form):
    """Constant planes (a different constant per plane, one of them -0.0): sigma = 0 and the output is bitwise the
    clean gather's."""
    from mtl_das_pytorch_amd.ops import functional as F
    kind, a, b = form
    Cin, taps, off = (1, a, b) if kind == "pack" else (a, 0, 0)
    H, W, N = 9, 13, 5
    X = (torch.arange(N * Cin).view(N, Cin, 1, 1) * 17.3 - 40.0).expand(N, Cin, H, W).contiguous()
    X[0] = -0.0
    c = Case(H, W, Cin, taps, off, False, X=X, rows=(4, 0, 4), snr=(-5.0, -5.0))
    assert (c.P[[4, 0]] == 0).all()
    lab = torch.zeros(N, 2, dtype=torch.int64, device="cuda")
    ref, _ = F.gather_batch(X.cuda(), lab, torch.tensor([4, 0, 4]).cuda(), taps=taps, off=off)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.o), _bits(ref.cpu()))
    assert torch.equal(c.y, X[[4, 0, 4]]) and torch.equal(c.y.view(torch.int32), X[[4, 0, 4]].view(torch.int32))


def test_draws_streams_and_advance():
    from mtl_das_pytorch_amd.ops import functional as F
    a = Case(7, 10, 1, 3, 1, False, draw=DRAW)
    b = Case(7, 10, 1, 3, 1, False, draw=DRAW + 1)
    e = Case(7, 10, 1, 3, 1, False, draw=DRAW, stream=2)
    b.check()
    e.check()
    assert (a.y != b.y).all() and (a.y != e.y).all() and (b.y != e.y).all()
    F.noise_advance(a.draw)  # the advance launch adds exactly 1 (int64: past 2^32)
    torch.cuda.synchronize()
    assert a.draw.item() == DRAW + 1
    c = Case(7, 10, 1, 3, 1, False, draw=2 ** 32 - 1)
    F.noise_advance(c.draw)
    assert c.draw.item() == 2 ** 32
    # the launch reads the draw from the device: the advanced tensor gives draw d + 1's noise
    again = torch.full_like(a.dbg, SENT)
    F.gather_batch_noise(a.Xc.cuda(), torch.zeros(5, 2, dtype=torch.int64, device="cuda"),
                         torch.tensor(a.rows).cuda(), a.P, a.snr, a.draw, SEED, taps=3, off=1, dbg=again)
    assert torch.equal(again[:210].view(3, 1, 7, 10).cpu(), b.y)


@pytest.mark.parametrize("form", [("pack", 3, 1), ("chan", 2, 0)], ids=["pack3_1", "chan2"])
def test_per_sample_snr_draw(form):
    """lo != hi: each sample's sigma^2 / P is 10^(-snr_s / 10) of the definition's level (1e-5 relative), shared by
    its channels.  sigma is the least-squares slope of (y - x) on the definition's g over the plane; x is of sigma's
    size, so the fp32 rounding of y (2^-24 |y| per element, averaged over the plane) is far inside the bound."""
    kind, a, b = form
    Cin, taps, off = (1, a, b) if kind == "pack" else (a, 0, 0)
    H, W, N = 9, 13, 5
    X = torch.randn(N, Cin, H, W, generator=torch.Generator().manual_seed(4))
    c = Case(H, W, Cin, taps, off, True, X=X, snr=(0.0, 20.0))
    _, x, _, g = c.reference()
    level = nz.sample_snr(c.rows, 0.0, 20.0, SEED, DRAW)
    assert level[0] == level[2] != level[1]
    n = c.y.double().numpy() - x
    sig = (n * g).sum((2, 3)) / (g * g).sum((2, 3))
    ratio = sig ** 2 / c.P.double().cpu().numpy()[c.rows]
    want = (10.0 ** (-level / 10.0))[:, None]
    print("sigma^2 / P relative error", np.abs(ratio / want - 1).max())
    assert np.abs(ratio / want - 1).max() <= 1e-5


def test_launcher_refuses_what_it_cannot_serve():
    from mtl_das_pytorch_amd.ops.hip import lib, stream
    c = Case(7, 10, 1, 3, 1, False)
    X, idx = c.Xc.cuda(), torch.tensor(c.rows).cuda()
    lab = torch.zeros(5, 2, dtype=torch.int64, device="cuda")
    lab_out = torch.zeros(3, 2, dtype=torch.int64, device="cuda")
    nz = {"power": c.P.data_ptr(), "snr": c.snr.data_ptr(), "draw": c.draw.data_ptr(), "seed_lo": 1, "seed_hi": 2,
          "noise_stream": 0}
    d = {"X": X.data_ptr(), "idx": idx.data_ptr(), "lab": lab.data_ptr(), "lab_w": 2, "out": c.out.data_ptr(),
         "lab_out": lab_out.data_ptr(), "B": 3, "Cin": 1, "H": 7, "W": 10, "taps": 3, "off": 1, "noise": nz}
    c.out.fill_(SENT)
    for bad in ({"noise": {**nz, "power": 0}}, {"Cin": 9, "taps": 0}, {"taps": 9}, {"Cin": 2},
                {"noise": {**nz, "snr": 0}}, {"noise": {**nz, "draw": 0}}):
        with pytest.raises(RuntimeError, match="rc=-2"):
            lib().gather_batch(stream(), {**d, **bad})
    torch.cuda.synchronize()
    assert (c.out.float() == SENT).all()  # a refused noisy launch has not run the clean kernel either
