"""tests/bwd_ref.py (the fp64 reference of the fused backward join) against fp64 ``torch.autograd`` on the CPU:
the join for every conv geometry of the GPU tests with 0-3 added sources, the tail for every kind with one and
several gradient sources, and the share of mask-ambiguous elements in every input the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

import bwd_ref as R

RTOL = 1e-10


def close(got, ref, what):
    err = (got - ref).abs().max().item() / ref.abs().max().clamp_min(1e-300).item()
    assert err <= RTOL, (what, err)


@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 2, 1), (1, 2, 0)])
@pytest.mark.parametrize("nsrc", [0, 1, 3])
def test_join_matches_autograd(k, s, p, nsrc):
    gen = torch.Generator().manual_seed(5)
    B, H, W, Ci, Co = 2, 17, 42, 8, 16
    w = (torch.randn(Co, Ci, k, k, generator=gen) / 8).bfloat16()
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x, w.double(), None, s, p)
    dy = torch.randn(out.shape, generator=gen).bfloat16()
    srcs = [torch.randn(B, H, W, Ci, generator=gen).bfloat16() for _ in range(nsrc)]
    loss = (out * dy.double()).sum()
    for t in srcs:
        loss = loss + (x * t.double().permute(0, 3, 1, 2)).sum()
    loss.backward()
    got = R.join(w.float(), dy.permute(0, 2, 3, 1).contiguous(), (H, W), s, p, srcs)
    close(got, x.grad.permute(0, 2, 3, 1), "join")


def _autograd_tail(name, t, srcs, gscale):
    """The tail's forward in fp64 with the batch statistics as functions of y, differentiated by autograd."""
    kind, proj = R.KINDS[name]
    leaf = {n: t[n].double().requires_grad_(True) for n in ("y", "r", "y2", "gamma", "beta", "gamma2", "beta2")}

    def bn(v, gamma, beta):
        mean = v.mean((0, 1, 2))
        xh = (v - mean) / torch.sqrt(v.var((0, 1, 2), unbiased=False) + R.EPS)
        return gamma * xh + beta
    z = bn(leaf["y"], leaf["gamma"], leaf["beta"])
    z.retain_grad()
    if kind == R.ACT_NONE:
        out = z
    elif kind == R.ACT_RELU:
        out = F.relu(z)
    elif kind == R.ACT_SIGMOID:
        out = torch.sigmoid(z)
    elif kind == R.SIGMUL:
        out = torch.sigmoid(z) * leaf["r"]
    elif kind == R.ADD_RELU:
        out = F.relu(z + (bn(leaf["y2"], leaf["gamma2"], leaf["beta2"]) if proj else leaf["r"]))
    else:
        out = F.max_pool2d(F.relu(z).permute(0, 3, 1, 2), 2, ceil_mode=True).permute(0, 2, 3, 1)
    (out * sum(s.double() for s in srcs)).sum().backward()
    g = {n: v.grad for n, v in leaf.items()}
    g["z"] = z.grad
    return g


@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("name", list(R.KINDS))
def test_tail_matches_autograd(name, nsrc):
    kind, proj = R.KINDS[name]
    B, H, W, C = 2, 7, 9, 8  # odd H and W: ceil-mode pool windows
    t = R.tail_inputs(3, B, H, W, C)
    # exact fp64 constants, so that the reference and autograd differentiate the same function
    t["k"] = R.batch_consts(t["y"], t["gamma"], t["beta"], dtype=torch.float64)
    t["k2"] = R.batch_consts(t["y2"], t["gamma2"], t["beta2"], dtype=torch.float64)
    gen = torch.Generator().manual_seed(11)
    gs = (B, (H + 1) // 2, (W + 1) // 2, C) if kind == R.POOL_RELU else (B, H, W, C)
    srcs = [torch.randn(gs, generator=gen).bfloat16() for _ in range(nsrc)]
    ag = _autograd_tail(name, t, srcs, 1.0)
    o = R.kind_tail(name, t, srcs if nsrc > 1 else srcs[0], gscale=0.5)
    close(o["dz"], ag["z"], "dz")
    close(o["sdz"], ag["beta"], "sum dz")
    close(o["sdzx"], ag["gamma"], "sum dz xhat")
    close(o["dy"], ag["y"], "dy")
    close(o["dgamma"], 0.5 * ag["gamma"], "dgamma")
    close(o["dbeta"], 0.5 * ag["beta"], "dbeta")
    if kind == R.SIGMUL or (kind == R.ADD_RELU and not proj):
        close(o["side"], ag["r"], "side")
    else:
        assert o["side"] is None
    if proj:
        close(o["sdzx2"], ag["gamma2"], "sum dz xhat2")
        close(o["dy2"], ag["y2"], "dy2")
        close(o["dgamma2"], 0.5 * ag["gamma2"], "dgamma2")
        close(o["dbeta2"], 0.5 * ag["beta2"], "dbeta2")
    else:
        assert o["dy2"] is None
    m, amb = R.kind_mask(name, t)
    assert (amb is None) == (name in ("none", "sigmoid", "sigmul"))


def test_pool_mask_ties_and_ambiguity():
    """Equal values in a window (bf16 inputs repeat): the first in row-major order takes the gradient, as in the
    kernel and in torch; a window whose two largest values are closer than AMBIG marks both as ambiguous."""
    y = torch.tensor([[1.0, 1.0, 2.0, 2.00005], [0.5, 1.0, -1.0, 0.0], [-1.0, -2.0, 3.0, 0.0]]).view(1, 3, 4, 1)
    k = torch.tensor([1.0, 0.0, 0.0, 1.0]).view(4, 1)
    m, amb = R.mask(R.POOL_RELU, y, k)
    assert m.view(3, 4).tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert amb.view(3, 4).tolist() == [[False, False, True, True], [False] * 4, [False] * 4]


AMBIG_SHARE = 5e-4  # at most 0.05 % of the elements may have a mask the fp32 kernels can decide either way


def test_ambiguous_share_of_the_gpu_inputs():
    worst = 0.0
    for seed in R.JOIN_SEEDS:
        t = R.tail_inputs(seed, *R.BASE, 32)
        for name in R.JOIN_KINDS:
            _, amb = R.kind_mask(name, t)
            share = amb.double().mean().item()
            worst = max(worst, share)
            assert share <= AMBIG_SHARE, (seed, name, share)
            assert not R.kind_mask(name, t, R.JOIN_MARGIN)[1].any(), (seed, name)
    for seed, B, H, W, C, kinds in R.TAIL_INPUTS:
        t = R.tail_inputs(seed, B, H, W, C)
        for name in kinds:
            _, amb = R.kind_mask(name, t)
            if amb is not None:
                share = amb.double().mean().item()
                worst = max(worst, share)
                assert share <= AMBIG_SHARE, (seed, name, share)
    print(f"worst ambiguous share {worst:.2e}")
