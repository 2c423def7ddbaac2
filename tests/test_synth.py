"""On-device synthetic generator (csrc/synth.hip) against the torch implementation of the same
physical model (data/synthetic.py), a NumPy Philox-4x32-10 reference and, element by element, the fp64 reference of
tests/synth_ref.py (clean signal, noise, launch independence, launcher refusals)."""
import numpy as np
import pytest
import torch

import synth_ref as S
from mtl_das_pytorch_amd.data.synthetic import generate

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_np(ctr: np.ndarray, key: int) -> np.ndarray:
    """Philox-4x32-10 on uint32 counters [n, 4] (Salmon et al., SC'11), vectorised in NumPy."""
    c = ctr.astype(np.uint64)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[:, 0]
        p1 = np.uint64(M1) * c[:, 2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c = np.stack([hi1 ^ c[:, 1] ^ k0, lo1, hi0 ^ c[:, 3] ^ k1, lo0], 1)
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c.astype(np.uint32)


def test_philox_known_answers():
    """Random123's published Philox-4x32-10 known-answer vectors."""
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32)
    keys = [0, 0xFFFFFFFFFFFFFFFF, (0x299F31D0 << 32) | 0xA4093822]
    want = [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    for i in range(3):
        assert philox_np(ctr[i:i + 1], keys[i])[0].tolist() == want[i]


@pytest.mark.gpu
def test_philox_device_matches_numpy():
    from mtl_das_pytorch_amd.ops.hip import lib
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    key = 0x1234567890ABCDEF
    c = torch.from_numpy(ctr.view(np.int32)).cuda()
    out = torch.empty_like(c)
    lib().philox_kat(c.data_ptr(), key, out.data_ptr(), 1000, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), philox_np(ctr, key))


@pytest.mark.gpu
@pytest.mark.parametrize("in_channels", [1, 3])
def test_hip_generator_clean_signal_matches_torch(in_channels):
    """Same seed -> same labels and per-sample scalars; the clean signal agrees with the torch model to fp32
    rounding (rare isolated points sit on the discontinuity of remainder(tau, period), where a last-bit
    difference of tau picks the other branch)."""
    n = 64
    xh, dh, eh = generate(n, seed=5, device="cuda", in_channels=in_channels, backend="hip", noise=False)
    xt, dt, et = generate(n, seed=5, device="cuda", in_channels=in_channels, backend="torch", noise=False)
    assert torch.equal(dh, dt) and torch.equal(eh, et)
    diff = (xh - xt).abs()
    scale = xt.abs().amax()
    frac_bad = (diff > 1e-3 * scale).float().mean().item()
    assert frac_bad < 1e-4, frac_bad
    assert (diff.median() / scale).item() < 1e-6


@pytest.mark.gpu
def test_hip_generator_noise_statistics_and_determinism():
    """The noise is N(0, sigma_s^2) with sigma_s set by the drawn SNR, reproducible and independent per sample."""
    n = 256
    x1, d, e = generate(n, seed=9, device="cuda")
    x2, _, _ = generate(n, seed=9, device="cuda")
    assert torch.equal(x1, x2)  # deterministic
    x3, _, _ = generate(n, seed=10, device="cuda")
    assert not torch.equal(x1, x3)
    clean, _, _ = generate(n, seed=9, device="cuda", noise=False)
    noise = (x1 - clean) / 100.0
    p_sig = (clean / 100.0).pow(2).mean((1, 2, 3)).clamp_min(1e-12)
    g = torch.Generator().manual_seed(9)  # replay the CPU draws up to the SNR
    torch.randint(0, 16, (n,), generator=g), torch.randint(0, 2, (n,), generator=g)
    torch.rand(n, generator=g), torch.rand(n, generator=g), torch.rand(n, 4, generator=g)
    snr = (torch.rand(n, generator=g) * 14.0 + 6.0).cuda()
    sigma = torch.sqrt(p_sig / 10.0 ** (snr / 10.0))
    z = noise / sigma.view(n, 1, 1, 1)
    assert abs(z.mean().item()) < 5e-3
    assert abs(z.std().item() - 1.0) < 5e-3
    zz = z.flatten().double()
    assert abs((zz ** 4).mean().item() - 3.0) < 0.05  # Gaussian kurtosis
    # neighbouring elements and samples uncorrelated
    assert abs((z[:, :, :, 1:] * z[:, :, :, :-1]).mean().item()) < 5e-3
    assert abs((z[1:] * z[:-1]).mean().item()) < 5e-3


# ---------------------------------------------------------------------------------------------------
# The generator element by element against the fp64 reference of tests/synth_ref.py.
#
# Clean signal: |out / 100 - clean| <= T |envelope| wherever the element is not ambiguous (tau within 2e-6 of a branch
# of the step or the remainder; at most 1e-4 of a case's elements, asserted on the CPU below), |envelope| there.
# T_TORCH is the worst such ratio of the fp32 TORCH backend -- a second, independent fp32 evaluation of the same
# formula -- against the reference over the committed cases, measured on the CPU: 1.61e-5 (100x250; 7.1e-6 at 9x7,
# 1.6e-6 at 5x7, 2.7e-7 at 1x9).  T is 4 x that: the device's expf / cosf / sinf are a few ulp where libm's are one,
# in an argument that reaches about 55 rad.
# Noise: |out / 100 - (clean + sigma g)| <= 1e-5 (|envelope| + sigma (1 + |g|)) + T |envelope|, the 1e-5 being the
# project's bound of this Box-Muller arithmetic (tests/test_noise_gpu.py), with the fp32 tree reduction of the
# signal power inside it.
T_TORCH = 1.61e-5
T_CLEAN = 4 * T_TORCH
NOISE_BOUND = 1e-5
SENT = -12288.0


def _clean_ratio(out100, ref):
    """(worst |err| / |envelope| over the unambiguous elements, the ambiguous share); asserts the ambiguous elements'
    own bound."""
    err = np.abs(np.asarray(out100, dtype=np.float64) / 100.0 - ref["clean"])
    amb = ref["ambiguous"]
    assert (err[amb] <= ref["env"][amb]).all()
    ok = ~amb
    return float((err[ok] / ref["env"][ok]).max()), float(amb.mean())


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_fp64_reference_against_torch_backend(case):
    """CPU: the reference's clean signal against the torch backend, the ambiguous share of every committed case, and
    the measurement T rests on."""
    H, W, C, n = case
    p, d, e = S.params(n, seed=5)
    assert set(e[:2].tolist()) == {0, 1} and d[0] == 0 and d[1] == 15
    ref = S.reference(p, C, H, W)
    xt, _, _ = generate(n, seed=5, in_channels=C, height=H, width=W, distance=d, event=e, backend="torch", noise=False)
    ratio, share = _clean_ratio(xt.numpy(), ref)
    print(f"{S.case_id(case)}: torch backend worst |err| / |envelope| = {ratio:.3e} (T_TORCH {T_TORCH:.1e}, "
          f"T {T_CLEAN:.2e}); ambiguous share {share:.2e} (cap {S.AMBIGUOUS_CAP:.0e})")
    assert share <= S.AMBIGUOUS_CAP
    assert ratio <= T_TORCH * 1.25   # (another libm may differ in the last digit; the kernel's bound is 4 x T_TORCH)
    assert np.abs(ref["clean"]).max() <= np.abs(ref["env"]).max() and (np.abs(ref["clean"]) <= ref["env"] * (1 + 1e-12)).all()


def test_reference_gaussian_layout():
    """The layout of synth_ref.gaussian spelled out for single elements, and its moments."""
    key, s0 = S.KEYS[1], 5
    g = S.gaussian(2, 3, 5, 7, key, s0)
    for (s, c, h, w) in ((0, 0, 0, 0), (1, 2, 3, 4), (1, 1, 4, 6)):
        e = h * 7 + w
        r = philox_np(np.array([[e // 4, c, s0 + s, 0]], dtype=np.uint32), key)[0]
        pair = r[:2] if e % 4 < 2 else r[2:]
        u0, u1 = ((float(v >> 8) + 1.0) * 2.0 ** -24 for v in pair)
        m, a = np.sqrt(-2.0 * np.log(u0)), 2.0 * np.pi * u1
        assert g[s, c, h, w] == pytest.approx(m * np.cos(a) if e % 2 == 0 else m * np.sin(a), rel=1e-13, abs=1e-15)
    big = S.gaussian(4, 1, 100, 250, S.KEYS[0], 0)
    assert abs(big.mean()) < 1e-2 and abs(big.std() - 1.0) < 1e-2


def _launch(p, C, H, W, noise, key=0, sample0=0, n=None, row0=0, out=None):
    """One synth_das launch on rows [row0, row0 + n) of the device parameters ``p``; returns (out [n, C, H, W] on the
    CPU, the flat device buffer with its sentinel tail)."""
    from mtl_das_pytorch_amd.ops.hip import lib, stream
    n = p.shape[0] - row0 if n is None else n
    numel = n * C * H * W
    buf = torch.full((numel + 64,), SENT, device="cuda") if out is None else out
    lib().synth_das(stream(), {"params": p.data_ptr() + row0 * 9 * 4, "out": buf.data_ptr(), "n": n, "C": C, "H": H,
                               "W": W, "noise": noise, "key": key, "sample0": sample0})
    torch.cuda.synchronize()
    return buf[:numel].view(n, C, H, W).cpu(), buf


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_generator_against_fp64(case):
    H, W, C, n = case
    p, _, _ = S.params(n, seed=5)
    pd = p.cuda()
    clean, buf = _launch(pd, C, H, W, noise=0)
    assert (buf[clean.numel():] == SENT).all()
    ref = S.reference(p, C, H, W)
    ratio, share = _clean_ratio(clean.numpy(), ref)
    assert share <= S.AMBIGUOUS_CAP
    worst_noise = 0.0
    for key in S.KEYS:
        for s0 in S.SAMPLE0:
            y, buf = _launch(pd, C, H, W, noise=1, key=key, sample0=s0)
            assert (buf[y.numel():] == SENT).all()
            r = S.reference(p, C, H, W, key, s0)
            err = np.abs(y.double().numpy() / 100.0 - r["noisy"])
            bound = NOISE_BOUND * (r["env"] + r["sigma"] * (1.0 + np.abs(r["g"]))) + T_CLEAN * r["env"]
            ok = ~r["ambiguous"]
            worst_noise = max(worst_noise, float((err[ok] / bound[ok]).max()))
    print(f"{S.case_id(case)}: worst clean |err| / |envelope| = {ratio:.3e} (T {T_CLEAN:.2e}); worst noise "
          f"|err| / bound = {worst_noise:.3e}; ambiguous share {share:.2e}")
    assert ratio <= T_CLEAN
    assert worst_noise <= 1.0


@pytest.mark.gpu
def test_generator_launch_independence():
    """Six samples in one launch, and as rows 0-1 (sample0 = 0) and rows 2-5 (the parameter pointer advanced,
    sample0 = 2): bit-equal."""
    H, W, C = 9, 7, 3
    p = S.params(6, seed=8)[0].cuda()
    key = S.KEYS[1]
    one, _ = _launch(p, C, H, W, 1, key, 0)
    a, _ = _launch(p, C, H, W, 1, key, 0, n=2)
    b, _ = _launch(p, C, H, W, 1, key, 2, n=4, row0=2)
    two = torch.cat([a, b])
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    assert not torch.equal(one[2:], _launch(p, C, H, W, 1, key, 0, n=4, row0=2)[0])  # sample0 is in the counter


@pytest.mark.gpu
def test_generator_launcher_refusals():
    """csrc/synth.hip launch_synth_das returns before the launch on n <= 0, a zero dimension and null pointers."""
    from mtl_das_pytorch_amd.ops.hip import lib, stream
    p = S.params(3, seed=5)[0].cuda()
    out = torch.full((3 * 5 * 7 + 64,), SENT, device="cuda")
    d = {"params": p.data_ptr(), "out": out.data_ptr(), "n": 3, "C": 1, "H": 5, "W": 7, "noise": 1, "key": 1, "sample0": 0}
    for bad in ({"n": 0}, {"n": -1}, {"C": 0}, {"H": 0}, {"W": 0}, {"params": 0}, {"out": 0}):
        with pytest.raises(RuntimeError, match="rc=-2"):
            lib().synth_das(stream(), {**d, **bad})
    torch.cuda.synchronize()
    assert (out == SENT).all()


@pytest.mark.gpu
def test_hip_generator_trains_like_torch_data():
    """The engine learns the event task from HIP-generated data as it does from torch-generated data."""
    from mtl_das_pytorch_amd.engine.mtl import MTLProgram
    from mtl_das_pytorch_amd.engine.step import StepRunner
    from mtl_das_pytorch_amd.models import MTL_Net
    torch.manual_seed(0)
    X, d, e = generate(512, seed=3, device="cuda")
    lab = torch.stack([d, e], 1)
    prog = MTLProgram(MTL_Net(), 32, "cuda")
    prog.set_optimizer(weight_decay=0.0)
    run = StepRunner(prog, X, lab)
    run.set_lr(1e-3)
    for ep in range(3):
        for i in range(16):
            run.train_step(torch.arange(32 * i, 32 * (i + 1), device="cuda"))
    Xt, dt, et = generate(256, seed=4, device="cuda")
    run.set_eval_source(Xt, torch.stack([dt, et], 1))
    run.reset_metrics()
    for i in range(8):
        run.eval_step(torch.arange(32 * i, 32 * (i + 1), device="cuda"))
    m = prog.metrics.cpu()
    assert m[-1, 2].item() == 256
    assert m[-1, 1].item() / 256 > 0.8  # held-out event accuracy
