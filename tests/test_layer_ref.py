"""tests/layer_ref.py on the CPU: every reference against fp64 autograd of the single op, a clean emulation of the
engine (fp32 ``F.conv2d`` of the bf16 operands rounded once to bf16, fp32 tail math) inside every bound, and ten
planted faults, each reported by the bound meant for it (the assertion names the Checker kind: without that check
the fault test fails)."""
import pytest
import torch
import torch.nn.functional as F

import bwd_ref as BR
import fwd_ref as FR
import layer_ref as L
import pool_ref as PR

B, H, W = 2, 9, 21
EPS = 1e-5


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def bf(t):
    return t.bfloat16().float()


# name -> (segments of the input, Co or member widths of a fused head, kernel, stride, padding, groups)
CONVS = {
    "3x3": ((32,), 48, (3, 3), 1, 1, 1),
    "3x3 s2": ((32,), 48, (3, 3), 2, 1, 1),
    "1x7": ((32,), 48, (1, 7), 1, (0, 3), 1),
    "7x1": ((32,), 48, (7, 1), 1, (3, 0), 1),
    "1x1 C64": ((64,), 48, (1, 1), 1, 0, 1),
    "3x3 C64": ((64,), 32, (3, 3), 1, 1, 1),
    "1x1 s2": ((32,), 48, (1, 1), 2, 0, 1),
    "two segments": ((16, 16), 48, (3, 3), 1, 1, 1),
    "two groups": ((32,), 48, (3, 3), 1, 1, 2),
    "fused head": ((64,), (16, 24, 16), (1, 1), 1, 0, 1),
}


class Conv:
    """The operands of one case (per group): bf16-valued segments, fp32 weights (one per member), a bf16 dy and two
    bf16 gradient sources of the input's shape; ``emu*``: what a clean engine stores."""

    def __init__(self, name):
        segs, co, k, s, p, G = CONVS[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        self.name, self.segs, self.k, self.s, self.p, self.G = name, segs, k, s, p, G
        self.members = co if isinstance(co, tuple) else (co,)
        Cs, Co = sum(segs), sum(self.members)
        K = k[0] * k[1] * Cs
        self.xs = [[bf(torch.randn(B, H, W, c, generator=g)) for c in segs] for _ in range(G)]
        self.ws = [[torch.randn(m, Cs, *k, generator=g) / K ** 0.5 for m in self.members] for _ in range(G)]
        y = F.conv2d(nchw(self.x(0)), bf(self.w(0)), None, s, p)
        self.dys = [bf(torch.randn(B, y.shape[2], y.shape[3], Co, generator=g)) for _ in range(G)]
        self.srcs = [[bf(torch.randn(B, H, W, Cs, generator=g)) for _ in range(2)] for _ in range(G)]

    def x(self, z, swap=False):
        s = self.xs[z]
        return torch.cat(s[::-1] if swap else s, -1)  # as the module concatenates its two inputs

    def w(self, z):
        return torch.cat(self.ws[z], 0)

    def emu_y(self, z, x=None, w=None):
        """(fp32 accumulators, the stored bf16 y) NHWC."""
        acc = nhwc(F.conv2d(nchw(self.x(z) if x is None else x), bf(self.w(z)) if w is None else w, None, self.s, self.p))
        return acc, acc.bfloat16()

    def emu_dx(self, z, nsrc):
        op = [H - ((self.dys[z].shape[1] - 1) * L._pair(self.s)[0] - 2 * L._pair(self.p)[0] + self.k[0]),
              W - ((self.dys[z].shape[2] - 1) * L._pair(self.s)[1] - 2 * L._pair(self.p)[1] + self.k[1])]
        g = nhwc(F.conv_transpose2d(nchw(self.dys[z]), bf(self.w(z)), None, self.s, self.p, op))
        for t in self.srcs[z][:nsrc]:
            g = g + t
        return g.bfloat16()

    def emu_dw(self, z, images=slice(None)):
        x = nchw(self.x(z))[images].requires_grad_(False)
        w = bf(self.w(z)).requires_grad_(True)
        F.conv2d(x, w, None, self.s, self.p).backward(nchw(self.dys[z])[images])
        return w.grad


@pytest.fixture(scope="module", params=list(CONVS))
def conv(request):
    return Conv(request.param)


def close(got, ref, what, rtol=1e-10):
    err = (got - ref).abs().max().item() / ref.abs().max().clamp_min(1e-300).item()
    assert err <= rtol, (what, err)


# ---------------------------------------------------------------------------------------------------
# 1. agreement with fp64 autograd
def test_conv_references_match_autograd(conv):
    for z in range(conv.G):
        x = nchw(conv.x(z)).double().requires_grad_(True)
        w = L.q(conv.w(z)).requires_grad_(True)
        y = F.conv2d(x, w, None, conv.s, conv.p)
        dy, srcs = conv.dys[z], conv.srcs[z]
        (y * nchw(dy).double()).sum().backward()
        f = L.conv_fwd(conv.x(z), conv.w(z), conv.s, conv.p)
        close(f["y"], nhwc(y.detach()), "y")
        close(f["abs"], nhwc(F.conv2d(x.detach().abs(), w.detach().abs(), None, conv.s, conv.p)), "abs y")
        assert f["n"] == conv.k[0] * conv.k[1] * sum(conv.segs)
        d = L.conv_dgrad(conv.w(z), dy, (H, W), conv.s, conv.p, srcs)
        close(d["g"], nhwc(x.grad) + srcs[0].double() + srcs[1].double(), "dx")
        assert bool((d["abs"] >= d["g"].abs() * (1 - 1e-12)).all())
        wg = L.conv_wgrad(conv.x(z), dy, w.shape, conv.s, conv.p)
        close(wg["dW"], w.grad, "dW")
        assert bool((wg["abs"] >= wg["dW"].abs() * (1 - 1e-12)).all())


def test_conv_bias_counts_as_an_addend():
    c = Conv("3x3")
    b = torch.randn(48)
    f = L.conv_fwd(c.x(0), c.w(0), 1, 1, bias=b)
    ref = F.conv2d(nchw(c.x(0)).double(), L.q(c.w(0)), b.double(), 1, 1)
    close(f["y"], nhwc(ref), "y + bias")
    assert f["n"] == 9 * 32 + 1


def test_bn_train_matches_torch():
    """Constants and running statistics (unbiased variance) against fp64 F.batch_norm in training mode."""
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B, H, W, 8, generator=g, dtype=torch.float64) * 2 + 0.3
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    rm, rv = torch.randn(8, generator=g).double(), torch.rand(8, generator=g).double() + 0.5
    ref = L.bn_train(y, y.abs(), 1, gamma, beta, EPS)
    rm1, rv1 = rm.clone(), rv.clone()
    out = F.batch_norm(nchw(y), rm1, rv1, gamma.double(), beta.double(), True, 0.1, EPS)
    close(nhwc(out), y * ref["k"][0] + ref["k"][1], "BN(y)")
    m, v = FR.running(rm, rv, ref["k"][2], ref["var"], ref["count"], 0.1)
    close(m, rm1, "running mean")
    close(v, rv1, "running var")
    ev = L.bn_eval(rm1, rv1, gamma, beta, EPS)
    out = F.batch_norm(nchw(y), rm1, rv1, gamma.double(), beta.double(), False, 0.1, EPS)
    close(nhwc(out), y * ev[0] + ev[1], "eval BN(y)")


def test_pool_references_match_autograd():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, H, W, 8, generator=g, dtype=torch.float64)
    xa = nchw(x).requires_grad_(True)
    ya = F.max_pool2d(xa, 3, 2)
    gs = [torch.randn(nhwc(ya).shape, generator=g, dtype=torch.float64) for _ in range(2)]
    (ya * nchw(gs[0] + gs[1])).sum().backward()
    y, am = L.maxpool_fwd(x)
    close(y, nhwc(ya.detach()), "max pool")
    close(L.maxpool_bwd(gs, am, H, W)["g"], nhwc(xa.grad), "max pool dx")
    xa = nchw(x).requires_grad_(True)
    ya = F.avg_pool2d(xa, 3, 1, 1)  # count_include_pad
    gs = [torch.randn(x.shape, generator=g, dtype=torch.float64) for _ in range(2)]
    (ya * nchw(gs[0] + gs[1])).sum().backward()
    close(L.avgpool_fwd(x), nhwc(ya.detach()), "avg pool")
    close(L.avgpool_bwd(gs)["g"], nhwc(xa.grad), "avg pool dx")


# ---------------------------------------------------------------------------------------------------
# 2. a clean emulation stays inside every bound
def emu_consts(acc, gamma, beta, rm0, rv0, momentum=0.1, images=slice(None), biased=False):
    """The engine's BN forward on its fp32 accumulators: row sums in fp32, totals and constants in fp64, published
    in fp32; the running statistics updated in fp32."""
    a = acc[images]
    N = a.numel() // a.shape[-1]
    s1 = a.sum(2).double().sum((0, 1))
    s2 = (a * a).sum(2).double().sum((0, 1))
    k, var = FR.bn_consts(torch.stack([s1, s2]), N, gamma, beta, EPS)
    unb = var if biased else var * N / (N - 1)
    m = FR.f32(momentum)
    rm = ((1 - m) * rm0.double() + m * k[2]).float()
    rv = ((1 - m) * rv0.double() + m * unb).float()
    return k.float(), rm, rv


def bn_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g),
            0.5 + torch.rand(C, generator=g))


def check_conv(chk, conv, z, y=None, dx=None, dw=None, x=None, per_member=True):
    """Every conv bound of one group against a stored y / dx / dW (the clean emulation where None)."""
    f = L.conv_fwd(conv.x(z) if x is None else x, conv.w(z), conv.s, conv.p)
    y = conv.emu_y(z)[1] if y is None else y
    c0 = 0
    for i, m in enumerate(conv.members if per_member else (sum(conv.members),)):
        sl = slice(c0, c0 + m)
        chk.acc("y", f"{conv.name} z{z} member {i} y", y[..., sl], f["y"][..., sl], f["abs"][..., sl], f["n"])
        c0 += m
    for nsrc in (0, 2):
        d = L.conv_dgrad(conv.w(z), conv.dys[z], (H, W), conv.s, conv.p, conv.srcs[z][:nsrc])
        chk.acc("dx", f"{conv.name} z{z} dx + {nsrc} sources", conv.emu_dx(z, nsrc) if dx is None else dx,
                d["g"], d["abs"], d["n"])
    wg = L.conv_wgrad(conv.x(z), conv.dys[z], conv.w(z).shape, conv.s, conv.p)
    chk.l2("dW", f"{conv.name} z{z} dW", conv.emu_dw(z) if dw is None else dw, wg["dW"])
    return f


def test_clean_conv_emulation_inside_bounds(conv):
    chk = L.Checker()
    for z in range(conv.G):
        f = check_conv(chk, conv, z)
        acc, _ = conv.emu_y(z)
        gamma, beta, rm0, rv0 = bn_params(acc.shape[-1], 5 + z)
        k, rm, rv = emu_consts(acc, gamma, beta, rm0, rv0)
        ref = L.bn_train(f["y"], f["abs"], f["n"], gamma, beta, EPS)
        chk.bn_training(f"{conv.name} z{z} BN", k, ref, beta, run=(rm, rv, rm0, rv0, 1, 0))
    chk.done()


def test_clean_nol_emulation_inside_bounds():
    """A normalise-on-load consumer: the operand rebuilt in fp32 (fused multiply-add or not), conv in fp32."""
    c = Conv("3x3")
    d = BR.tail_inputs(3, B, H, W, 32)
    k = d["k"]
    chk = L.Checker()
    ref = L.nol_conv_fwd(d["y"], k[0], k[1], L.ACT_RELU, c.w(0), 1, 1)
    for fused in (False, True):
        y32 = d["y"].float()
        v = torch.addcmul(k[1], y32, k[0]) if fused else y32 * k[0] + k[1]
        a = v.clamp_min(0).bfloat16().float()
        chk.true("operand within its ambiguity", bool(((a.double() == ref["operand"]) | ref["amb_map"]).all()))
        _, y = c.emu_y(0, x=a)
        chk.acc("nol y", f"fused {fused}", y, ref["y"], ref["abs"], ref["n"], ref["amb"])
    chk.done()


TAIL_KINDS = list(BR.KINDS)


def emu_tail_fwd(name, t):
    kind, proj = BR.KINDS[name]
    k, k2 = t["k"], t["k2"]
    v = t["y"].float() * k[0] + k[1]
    if kind == L.ACT_RELU:
        v = v.clamp_min(0)
    elif kind == L.ACT_SIGMOID:
        v = torch.sigmoid(v)
    elif kind == L.SIGMUL:
        v = torch.sigmoid(v) * t["r"].float()
    elif kind == L.ADD_RELU:
        v = (v + (t["y2"].float() * k2[0] + k2[1] if proj else t["r"].float())).clamp_min(0)
    elif kind == L.POOL_RELU:
        v = FR.pool2x2_ceil(v.clamp_min(0))
    return v.bfloat16()


def tail_args(name, t):
    kind, proj = BR.KINDS[name]
    r = t["y2"] if proj else (t["r"] if kind in (L.SIGMUL, L.ADD_RELU) else None)
    return kind, r, (t["k2"] if proj else None), (t["gamma2"] if proj else None)


def emu_tail_bwd(name, t, g, flip=None):
    """fp32 closed-form tail backward; ``flip`` [B, H, W] bool inverts the ReLU mask of those pixels."""
    kind, r, k2, gamma2 = tail_args(name, t)
    k = t["k"]
    y = t["y"].float()
    z = y * k[0] + k[1]
    n = y.numel() // y.shape[-1]
    if kind == L.POOL_RELU:
        g = BR.up(g, H, W)
        m = BR.mask(kind, t["y"], k)[0].float()
    elif kind == L.ACT_RELU:
        m = (z > 0).float()
    elif kind == L.ADD_RELU:
        m = ((z + (t["y2"].float() * k2[0] + k2[1] if k2 is not None else r.float())) > 0).float()
    elif kind == L.ACT_NONE:
        m = torch.ones_like(z)
    else:
        s = torch.sigmoid(z)
        m = s * (1 - s) * (r.float() if kind == L.SIGMUL else 1.0)
    if flip is not None:
        m = torch.where(flip[..., None], 1 - m, m)
    dz = g.float() * m
    xh = (y - k[2]) * k[3]
    sdz, sdzx = dz.double().sum((0, 1, 2)), (dz * xh).double().sum((0, 1, 2))
    out = {"dy": (t["gamma"] * k[3] * (dz - (sdz / n).float() - xh * (sdzx / n).float())).bfloat16(),
           "dgamma": sdzx.float(), "dbeta": sdz.float(), "side": None, "dy2": None, "dgamma2": None, "dbeta2": None}
    if kind == L.SIGMUL:
        out["side"] = (g.float() * torch.sigmoid(z)).bfloat16()
    elif kind == L.ADD_RELU and k2 is None:
        out["side"] = dz.bfloat16()
    elif kind == L.ADD_RELU:
        xh2 = (t["y2"].float() - k2[2]) * k2[3]
        sdzx2 = (dz * xh2).double().sum((0, 1, 2))
        out["dy2"] = (gamma2 * k2[3] * (dz - (sdz / n).float() - xh2 * (sdzx2 / n).float())).bfloat16()
        out["dgamma2"], out["dbeta2"] = sdzx2.float(), sdz.float()
    return out


def check_tail_bwd(chk, name, t, g, e):
    kind, r, k2, gamma2 = tail_args(name, t)
    o = L.tail_bwd(kind, t["y"], t["k"], t["gamma"], g, r, k2, gamma2)
    chk.tail_grads(name, o, e["dgamma"], e["dbeta"], e["dy"], e["side"], e["dy2"], e["dgamma2"], e["dbeta2"])
    if kind == L.ADD_RELU and k2 is None:  # the identity shortcut's gradient is dz itself: elementwise, one rounding
        chk.acc("side", name + " side", e["side"], o["side"], o["side"].abs(), 1, skip=o["amb"])
    return o


@pytest.mark.parametrize("name", TAIL_KINDS)
def test_clean_tail_emulation_inside_bounds(name):
    t = BR.tail_inputs(10, B, H, W, 48)
    gen = torch.Generator().manual_seed(4)
    kind = BR.KINDS[name][0]
    chk = L.Checker()
    kind_, r, k2, _ = tail_args(name, t)
    chk.ulp("tail", name, emu_tail_fwd(name, t), L.tail_fwd(kind, t["y"], t["k"], r, k2))
    gs = (B, (H + 1) // 2, (W + 1) // 2, 48) if kind == L.POOL_RELU else (B, H, W, 48)
    g = bf(torch.randn(gs, generator=gen))
    check_tail_bwd(chk, name, t, g, emu_tail_bwd(name, t, g))
    chk.done()


def pool_inputs(ties):
    g = torch.Generator().manual_seed(6)
    if ties:  # small integers: most windows hold their maximum more than once
        x = torch.randint(-2, 3, (B, H, W, 8), generator=g).float()
    else:
        x = bf(torch.randn(B, H, W, 8, generator=g))
    Ho, Wo = PR.max_out_hw(H, W)
    return x, [bf(torch.randn(B, Ho, Wo, 8, generator=g)) for _ in range(2)], \
        [bf(torch.randn(B, H, W, 8, generator=g)) for _ in range(2)]


def emu_max_bwd(x, gs, last=False):
    """fp32 max-pool backward; ``last``: ties go to the LAST maximum of a window (the planted fault)."""
    xs = x.flip(1, 2) if last else x
    if last:  # a flipped map has the same windows only if the map is covered exactly
        assert (H - 3) % 2 == 0 and (W - 3) % 2 == 0
    _, am = PR.max_fwd(xs.double())
    g = (gs[0] + gs[1])
    dx = PR.max_bwd(g.flip(1, 2) if last else g, am, H, W)
    return (dx.flip(1, 2) if last else dx).float().bfloat16()


def check_pools(chk, x, gmax, gavg, y_avg=None, dx_max=None):
    y, am = L.maxpool_fwd(x)
    chk.exact("max pool y", PR.max_fwd(x.double())[0].bfloat16(), y)
    d = L.maxpool_bwd(gmax, am, H, W)
    chk.acc("max pool dx", "max pool dx", emu_max_bwd(x, gmax) if dx_max is None else dx_max, d["g"], d["abs"], d["n"])
    ya = (F.avg_pool2d(nchw(x), 3, 1, 1)).permute(0, 2, 3, 1).bfloat16() if y_avg is None else y_avg
    chk.ulp("avg pool", "avg pool y", ya, L.avgpool_fwd(x))
    d = L.avgpool_bwd(gavg)
    dxa = nhwc(F.avg_pool2d(nchw(gavg[0] + gavg[1]), 3, 1, 1)).bfloat16()  # the backward is the same window sum / 9
    chk.acc("avg pool dx", "avg pool dx", dxa, d["g"], d["abs"], d["n"])


@pytest.mark.parametrize("ties", [False, True])
def test_clean_pool_emulation_inside_bounds(ties):
    chk = L.Checker()
    check_pools(chk, *pool_inputs(ties))
    chk.done()


# ---------------------------------------------------------------------------------------------------
# 3. planted faults
def reported(chk, kind):
    """The violated bounds of ``kind``; the Checker must assert at done()."""
    hits = [b for b in chk.bad if b[1] == kind]
    with pytest.raises(AssertionError):
        chk.done()
    return hits


def test_fault_edge_column_without_a_tap():
    """The last output column is computed with the bounds test off by one: the tap next to its padding tap is treated
    as padding too (1x7, padding 3: tap kw = 3 of output column Wo - 1 reads the last input column)."""
    c = Conv("1x7")
    acc, y = c.emu_y(0)
    w = bf(c.w(0)).clone()
    w[..., 3] = 0
    y = y.clone()
    y[:, :, -1] = c.emu_y(0, w=w)[1][:, :, -1]
    chk = L.Checker()
    check_conv(chk, c, 0, y=y)
    hits = reported(chk, "y")
    assert len(hits) == 1 and "member 0 y" in hits[0][0], chk.bad
    assert len(chk.bad) == 1


def test_fault_last_k_chunk_dropped():
    """The last 32 input channels never enter the reduction (a split K that loses its last chunk)."""
    c = Conv("3x3 C64")
    x = c.x(0).clone()
    x[..., -32:] = 0
    chk = L.Checker()
    check_conv(chk, c, 0, y=c.emu_y(0, x=x)[1])
    assert reported(chk, "y") and len(chk.bad) == 1, chk.bad


def test_fault_fused_head_slice_shifted():
    """The second member's slice [16, 40) of a fused 1x1 head lands 8 channels late."""
    c = Conv("fused head")
    y = c.emu_y(0)[1].clone()
    y[..., 16:40] = y[..., 16:40].roll(8, -1)
    chk = L.Checker()
    check_conv(chk, c, 0, y=y)
    hits = reported(chk, "y")
    assert [h[0] for h in hits] == ["fused head z0 member 1 y"], chk.bad


def test_fault_segments_swapped():
    c = Conv("two segments")
    chk = L.Checker()
    check_conv(chk, c, 0, y=c.emu_y(0, x=c.x(0, swap=True))[1])
    assert reported(chk, "y") and len(chk.bad) == 1, chk.bad


def test_fault_missing_image_in_weight_gradient():
    c = Conv("3x3")
    chk = L.Checker()
    check_conv(chk, c, 0, dw=c.emu_dw(0, images=slice(0, B - 1)))
    assert reported(chk, "dW") and len(chk.bad) == 1, chk.bad


@pytest.mark.parametrize("name", ["relu", "add", "add_proj"])
def test_fault_relu_mask_wrong_at_one_pixel_per_image(name):
    t = BR.tail_inputs(10, B, H, W, 48)
    g = bf(torch.randn(B, H, W, 48, generator=torch.Generator().manual_seed(4)))
    flip = torch.zeros(B, H, W, dtype=torch.bool)
    flip[:, 3, 5] = True
    chk = L.Checker()
    check_tail_bwd(chk, name, t, g, emu_tail_bwd(name, t, g, flip=flip))
    assert reported(chk, "dbeta sums") and [b for b in chk.bad if b[1] == "dgamma sums"], chk.bad
    assert [b for b in chk.bad if b[1] == "dy"], chk.bad
    if name == "add":
        assert [b for b in chk.bad if b[1] == "side" and "out of bound" in b[2]], chk.bad


def _bn_case():
    c = Conv("3x3")
    f = L.conv_fwd(c.x(0), c.w(0), c.s, c.p)
    acc, _ = c.emu_y(0)
    gamma, beta, rm0, rv0 = bn_params(48, 5)
    return acc, gamma, beta, rm0, rv0, L.bn_train(f["y"], f["abs"], f["n"], gamma, beta, EPS)


def test_fault_bn_mean_over_all_but_one_image():
    acc, gamma, beta, rm0, rv0, ref = _bn_case()
    good = emu_consts(acc, gamma, beta, rm0, rv0)[0]
    k = emu_consts(acc, gamma, beta, rm0, rv0, images=slice(0, B - 1))[0]
    k = torch.stack([good[0], beta - k[2] * good[0], k[2], good[3]])  # only the mean (and the shift built on it)
    chk = L.Checker()
    chk.bn_training("BN", k, ref, beta)
    assert reported(chk, "mean") and {b[1] for b in chk.bad} == {"mean", "shift"}, chk.bad


def test_fault_running_variance_biased():
    acc, gamma, beta, rm0, rv0, ref = _bn_case()
    k, rm, rv = emu_consts(acc, gamma, beta, rm0, rv0, biased=True)
    chk = L.Checker()
    chk.bn_training("BN", k, ref, beta, run=(rm, rv, rm0, rv0, 1, 0))
    assert reported(chk, "run_var") and len(chk.bad) == 1, chk.bad


def test_fault_average_pool_divides_by_valid_count():
    x, gmax, gavg = pool_inputs(False)
    ya = nhwc(F.avg_pool2d(nchw(x), 3, 1, 1, count_include_pad=False)).bfloat16()
    chk = L.Checker()
    check_pools(chk, x, gmax, gavg, y_avg=ya)
    assert reported(chk, "avg pool") and len(chk.bad) == 1, chk.bad


def test_fault_max_pool_backward_ties_to_the_last_maximum():
    x, gmax, gavg = pool_inputs(True)
    chk = L.Checker()
    check_pools(chk, x, gmax, gavg, dx_max=emu_max_bwd(x, gmax, last=True))
    assert reported(chk, "max pool dx") and len(chk.bad) == 1, chk.bad


@pytest.mark.parametrize("name", ["MTL", "multi_classifier"])
def test_models_at_init_stay_six_times_inside_the_cap(name):
    """The inputs of the layer-local GPU tests (fresh modules, ``generate(..., seed=11)``): in no BN layer are more
    than AMB_CAP / 6 of the outputs within bwd_ref.AMBIG of zero (fp32 modules on the CPU, 4 samples)."""
    from mtl_das_pytorch_amd.data.synthetic import generate
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(name).train()
    shares, near, total = [], 0, 0

    def hook(mod, inp, out):
        nonlocal near, total
        m = out.abs() < BR.AMBIG
        shares.append(float(m.float().mean()))
        near, total = near + int(m.sum()), total + out.numel()
    for b in model.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.register_forward_hook(hook)
    with torch.no_grad():
        model(generate(4, seed=11)[0])
    print(f"{name}: {len(shares)} BN layers, largest share {max(shares):.2e}, overall {near / total:.2e}")
    assert max(shares) <= L.AMB_CAP / 6, max(shares)


def test_ambiguity_cap():
    """More than AMB_CAP of a tensor left out of an elementwise check is itself a failure."""
    chk = L.Checker()
    ref = torch.ones(1000, dtype=torch.float64)
    skip = torch.zeros(1000, dtype=torch.bool)
    skip[:2] = True
    assert chk.acc("dx", "at the cap", ref.bfloat16(), ref, ref, 1, skip=skip) and not chk.bad
    skip[2] = True
    chk.acc("dx", "over the cap", ref.bfloat16(), ref, ref, 1, skip=skip)
    assert reported(chk, "cap")
