"""fp64 single-op references and derived bounds of the layer-local tests (tests/test_mtl_layer_local_gpu.py,
tests/test_inception_layer_local_gpu.py; checked on the CPU by tests/test_layer_ref.py).

Nothing here defines math of its own: the convolution is fwd_ref.conv2d_nhwc, the data gradient bwd_ref.join, the
weight gradient wpath_ref.wgrad_ref, the BN constants / running statistics / forward tails fwd_ref, the tail backward
and its masks bwd_ref, the Inception pools pool_ref.  This module adds the absolute-value companion of each
accumulation, the bounds derived from it and a Checker.  Plain torch ops on NHWC tensors; ``on(device)`` makes
bwd_ref compute where the operands live, so a whole layer at the benchmarked batch is referenced in fp64 on the GPU.

Bounds (none comes from what the kernels give):
  acc      a bf16 tensor from ONE fp32 accumulation of n addends and ONE rounding (forward y, dx, a gradient sum):
           |got - ref| <= 2^-8 |ref| + n 2^-24 absref + amb per element.  2^-8 |ref| is half a bf16 ulp at its largest;
           n 2^-24 sum|addends| is the worst case of an fp32 summation of n addends in ANY order (the products of two
           bf16 numbers are exact in fp32); amb is what operands on a bf16 rounding boundary may cost (fwd_ref.nol_conv),
           nonzero only for a normalise-on-load conv.
  ulp      tail and average-pool outputs: fwd_ref.one_ulp of the fp64 value of the engine's stored operands.
  consts   fwd_ref.Checker.consts / running_stats, widened by what the fp32 accumulators behind the totals may cost
           (stat_slack, from fwd_ref.randn_stat_bounds: again absref, nothing measured).
  l2       relative L2 of tests/test_mtl_layer_local_gpu.py TOL: dW 2e-4, d(gamma) / d(beta) 1e-5, dy / side / dhead 6e-3.
  sums     test_bwd_join_gpu's rule: |got_c - ref_c| <= 1e-4 sum|terms_c| + sum over mask-ambiguous elements of |term|.
  cap      at most AMB_CAP of a tensor's elements may be left out of an elementwise check as mask-ambiguous.
"""
from contextlib import contextmanager
from types import SimpleNamespace

import torch

import bwd_ref as BR
import fwd_ref as FR
import pool_ref as PR
import wpath_ref as WR
from fwd_ref import ACT_NONE, ACT_RELU, ACT_SIGMOID, ADD_RELU, POOL_RELU, SIGMUL  # noqa: F401

U24 = 2.0 ** -24
AMB_CAP = 0.002
TOL = {"dy": 6e-3, "dx": 6e-3, "dW": 2e-4, "dgamma": 1e-5, "dbeta": 1e-5, "side": 6e-3, "dhead": 6e-3}


@contextmanager
def on(device):
    """bwd_ref computes on ``device`` inside the block (it moves every operand to bwd_ref.DEVICE)."""
    old, BR.DEVICE = BR.DEVICE, device
    try:
        yield
    finally:
        BR.DEVICE = old


def q(t):
    """Rounded to bf16 (as the packed weight images are), in fp64."""
    return t.detach().float().bfloat16().double()


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def geometry(x_shape, w_shape, stride, padding):
    """The fwd_ref.FCase and wpath_ref.WCase of one group: x [B, H, W, Cs], w [Co, Cs, KH, KW]."""
    B, H, W, Cs = x_shape
    Co, Cw, KH, KW = w_shape
    assert Cw == Cs, (Cw, Cs)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    kw = dict(KH=KH, KW=KW, sh=sh, sw=sw, ph=ph, pw=pw)
    return FR.FCase("", B, H, W, Cs, Co, **kw), WR.WCase("", B, H, W, Cs, Co, **kw)


# ---------------------------------------------------------------------------------------------------
# convolution: forward, data gradient, weight gradient; each with its absolute-value companion
def conv_fwd(x, w, stride=1, padding=0, bias=None):
    """x [B, H, W, Cs] (bf16 values; a two-segment input concatenated as the module does), w [Co, Cs, KH, KW]
    (rounded to bf16 here), bias fp32 -> {"y", "abs" = conv(|x|, |w|) + |b|, "n" addends per output}."""
    w = q(w)
    c, _ = geometry(x.shape, w.shape, stride, padding)
    b = None if bias is None else bias.double()
    return {"y": FR.conv2d_nhwc(x, w, b, c), "abs": FR.conv2d_nhwc(x.abs(), w.abs(), None if b is None else b.abs(), c),
            "n": c.K + (bias is not None), "case": c}


def nol_conv_fwd(y_prev, scale, shift, kind, w, stride=1, padding=0, bias=None, slack=0.0):
    """A normalise-on-load conv of the producer's stored ``y_prev`` [B, H, W, Cs] with that BN's published fp32
    ``scale`` / ``shift`` [Cs]: conv_fwd's fields of the operand bf16(act(y * scale + shift)), plus ``amb`` (per
    output: what the operands on a rounding boundary may cost), ``operand`` and the operand's ``amb_map``."""
    a, amb = FR.nol_operand(y_prev, scale, shift, kind, slack=slack)
    w = q(w)
    c, _ = geometry(a.shape, w.shape, stride, padding)
    y, cost = FR.nol_conv(a, amb, w, c)
    T = FR.conv2d_nhwc(a.abs(), w.abs(), None, c)
    if bias is not None:
        y, T = y + bias.double(), T + bias.double().abs()
    return {"y": y, "abs": T, "n": c.K + (bias is not None), "amb": cost, "operand": a, "amb_map": amb, "case": c}


def conv_dgrad(w, dy, in_hw, stride=1, padding=0, sources=()):
    """g = conv_T(dy, w) + sum(sources) [B, H, W, Ci] (bwd_ref.join) with ``abs`` = conv_T(|dy|, |w|) + sum|sources|
    and ``n``: at most ceil(KH / sh) ceil(KW / sw) Co products reach one input pixel, plus the added sources."""
    (sh, sw) = _pair(stride)
    Co, _, KH, KW = w.shape
    wq = w.detach().float().bfloat16().float()
    return {"g": BR.join(wq, dy, in_hw, stride, padding, sources),
            "abs": BR.join(wq.abs(), dy.abs(), in_hw, stride, padding, [s.abs() for s in sources]),
            "n": -(-KH // sh) * -(-KW // sw) * Co + len(sources)}


def conv_wgrad(x, dy, w_shape, stride=1, padding=0):
    """dW [Co, Cs, KH, KW] = sum over the output pixels of x * dy (wpath_ref.wgrad_ref) and ``abs`` = sum |x * dy|."""
    _, c = geometry(x.shape, w_shape, stride, padding)
    assert tuple(dy.shape[1:3]) == (c.Ho, c.Wo), (dy.shape, c.Ho, c.Wo)
    x, dy = x.double(), dy.double()
    return {"dW": WR.to_nchw(WR.wgrad_ref(x, dy, c), c), "abs": WR.to_nchw(WR.wgrad_ref(x.abs(), dy.abs(), c), c),
            "n": c.M}


def acc_bound(ref, absref, n, amb=None):
    b = ref.abs() * 2.0 ** -8 + n * U24 * absref
    return b if amb is None else b + amb


# ---------------------------------------------------------------------------------------------------
# BN
def bn_train(y_ref, absref, n, gamma, beta, eps, amb=None):
    """Training-mode BN constants of the UNROUNDED reference ``y_ref`` [B, H, W, C] (the conv epilogue sums its fp32
    accumulators, not the stored bf16 y): {"k" [4, C] fwd_ref.bn_consts, "var", "count", "extra" [4, C] and "dstat" =
    (mean, variance) slack}: what the fp32 accumulation behind every y (worst case n 2^-24 absref, plus ``amb`` of a
    normalise-on-load conv) and the fp32 partial sums of the totals (fwd_ref.randn_stat_bounds) may move them."""
    N = y_ref.numel() // y_ref.shape[-1]
    k, var = FR.bn_consts(FR.totals(y_ref[None])[0], N, gamma, beta, eps)
    d1, d2 = FR.randn_stat_bounds(SimpleNamespace(M=N, K=n), {"y": y_ref[None], "T": absref[None]})
    if amb is not None:
        d1 = d1 + amb.sum((0, 1, 2))
        d2 = d2 + (2 * y_ref.abs() * amb + amb * amb).sum((0, 1, 2))
    extra, dstat = stat_slack(k, var, d1[0], d2[0], N, gamma, eps)
    return {"k": k, "var": var, "count": N, "extra": extra, "dstat": dstat}


def stat_slack(k, var, d1, d2, N, gamma, eps):
    """How far totals off by at most d1 = |d sum(y)|, d2 = |d sum(y^2)| move (scale, shift, mean, invstd) [4, C] and
    (mean, biased variance): mean d1 / N; var d2 / N + 2 |mean| dmean + dmean^2; invstd by evaluating it at both ends
    of the variance interval; scale |gamma| dinv; shift |mean| dscale + dmean (|scale| + dscale)."""
    sc, _, mu, inv = k.unbind(-2)
    dm = d1 / N
    dv = d2 / N + 2 * mu.abs() * dm + dm * dm
    hi = 1.0 / torch.sqrt((var - dv).clamp_min(0.0) + eps)
    lo = 1.0 / torch.sqrt(var + dv + eps)
    di = torch.maximum(hi - inv, inv - lo)
    ds = gamma.double().abs() * di
    return torch.stack([ds, mu.abs() * ds + dm * (sc.abs() + ds), dm, di], -2), (dm, dv)


def bn_eval(run_mean, run_var, gamma, beta, eps):
    return FR.eval_consts(run_mean, run_var, gamma, beta, eps)


def eval_nol_slack(y, k, beta):
    """Per operand element: how far an eval-mode normalise-on-load consumer's own fp32 constants (it publishes none)
    may move y * scale + shift from the fp64 constants ``k`` [4, C] -- fwd_ref.Checker.consts' rules for scale
    (5 2^-24 relative) and shift (8 2^-24 (|beta| + |mean scale|)), as tests/test_fwd_path_gpu.py applies them."""
    sc, mu = k[0].double(), k[2].double()
    return U24 * (5 * (y.double() * sc).abs() + 8 * (beta.double().abs() + (mu * sc).abs()))


def tail_fwd(kind, y, consts, r=None, consts2=None):
    """fwd_ref.tail_fwd on the engine's stored y and published fp32 constants [4, C]."""
    return FR.tail_fwd(kind, y, consts, r, consts2)


def tail_bwd(kind, y, consts, gamma, g, r=None, consts2=None, gamma2=None):
    """bwd_ref.tail plus ``gfull`` (the gradient every element's mask multiplies: |term| of a flipped mask is
    |gfull| resp. |gfull * xhat|) and ``share``, the mask-ambiguous share of the tensor."""
    o = BR.tail(kind, y, consts, gamma, g, r, consts2, gamma2)
    gs = g if isinstance(g, (list, tuple)) else [g]
    gsum = sum(BR.f64(t) for t in gs)
    o["gfull"] = BR.up(gsum, *y.shape[1:3]) if kind == POOL_RELU else gsum
    o["share"] = 0.0 if o["amb"] is None else float(o["amb"].double().mean())
    return o


# ---------------------------------------------------------------------------------------------------
# pools of Model C
def maxpool_fwd(x):
    return PR.max_fwd(x.double())


def maxpool_bwd(sources, am, H, W):
    gs = torch.stack([s.double() for s in sources])
    return {"g": PR.max_bwd(gs.sum(0), am, H, W), "abs": PR.max_bwd(gs.abs().sum(0), am, H, W), "n": 4 * len(sources)}


def avgpool_fwd(x):
    """Count-include-pad 3x3 / s1 / p1 average: always / 9."""
    return PR.avg_fwd(x.double())


def avgpool_bwd(sources):
    """n: 9 window positions per source, and the product with fp32(1 / 9) (two more roundings)."""
    gs = torch.stack([s.double() for s in sources])
    return {"g": PR.avg_bwd(gs.sum(0)), "abs": PR.avg_bwd(gs.abs().sum(0)), "n": 9 * len(sources) + 2}


# ---------------------------------------------------------------------------------------------------
class Checker(FR.Checker):
    """fwd_ref.Checker (exact / bounded / consts / running_stats / act: collects every violated bound, prints the worst
    value of each kind, asserts at ``done``) with the accumulation bound, the relative-L2 kinds, the per-channel sums
    and the ambiguity cap."""

    def __init__(self):
        super().__init__()
        self.share = 0.0

    def left_out(self, what, skip):
        """``skip``: the mask-ambiguous elements an elementwise check leaves out; at most AMB_CAP of the tensor."""
        s = float(skip.double().mean())
        self.share = max(self.share, s)
        self._note("ambiguous share", s)
        if not s <= AMB_CAP:
            self.bad.append((what, "cap", f"{s:.3e} of the elements mask-ambiguous (cap {AMB_CAP})"))
        return s <= AMB_CAP

    def _masked(self, what, got, ref, bound, skip):
        if skip is None:
            return got.double(), ref, bound
        self.left_out(what, skip)
        keep = ~skip.to(got.device)
        z = torch.zeros((), dtype=torch.float64, device=got.device)
        return (torch.where(keep, got.double(), z), torch.where(keep, ref.to(got.device), z),
                torch.where(keep, bound.to(got.device), z + 1.0))

    def acc(self, kind, what, got, ref, absref, n, amb=None, skip=None):
        """One fp32 accumulation, one bf16 rounding: acc_bound per element."""
        if tuple(got.shape) != tuple(ref.shape):
            self.bad.append((what, kind, "shape", tuple(got.shape), tuple(ref.shape)))
            return False
        g, r, b = self._masked(what, got, ref, acc_bound(ref, absref, n, amb), skip)
        return self.bounded(kind, what, g, r, b)

    def ulp(self, kind, what, got, ref, skip=None):
        """fwd_ref.one_ulp of the fp64 value."""
        g, r, b = self._masked(what, got, ref, FR.one_ulp(ref), skip)
        return self.bounded(kind, what, g, r, b)

    def l2(self, kind, what, got, ref, tol=None):
        tol = TOL[kind] if tol is None else tol
        ref = ref.to(got.device)
        if tuple(got.shape) != tuple(ref.shape) or not bool(torch.isfinite(got.float()).all()):
            self.bad.append((what, kind, "shape or non-finite"))
            return False
        v = ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
        self._note(kind + " rel L2", v)
        if not v < tol:
            self.bad.append((what, kind, f"rel L2 {v:.3e} (bound {tol:.0e})"))
        return v < tol

    def sums(self, kind, what, got, terms, ambt=None):
        """Per-channel sums ``got`` [C] against ``terms`` [..., C] (fp64); ``ambt``: |term| of the ambiguous elements."""
        red = tuple(range(terms.dim() - 1))
        ref, mag = terms.sum(red), terms.abs().sum(red)
        bound = 1e-4 * mag + (ambt.sum(red) if ambt is not None else 0.0)
        err = (got.double().to(ref.device) - ref).abs()
        self._note(kind + " sums err / sum|terms|", (err / mag.clamp_min(1e-300)).max().item())
        ok = bool((err <= bound).all())
        if not ok:
            c = int((err / bound.clamp_min(1e-300)).argmax())
            self.bad.append((what, kind + " sums", f"channel {c}: err {err[c].item():.3e} bound {bound[c].item():.3e}"))
        return ok

    # --- composites ---
    def bn_training(self, what, got_k, ref, beta, run=None, momentum=0.1):
        """Published constants ``got_k`` [4, C] against :func:`bn_train`'s ``ref``; ``run`` = (rm, rv, rm0, rv0, nbt,
        nbt0): the running statistics after the step and before it."""
        ok = self.consts(what, got_k, ref["k"], beta, ref["extra"])
        if run is not None:
            rm, rv, rm0, rv0, nbt, nbt0 = run
            ok &= self.running_stats(what, rm, rv, rm0, rv0, ref["k"][2], ref["var"], ref["count"], momentum, ref["dstat"])
            ok &= self.true(what + " num_batches_tracked", int(nbt) == int(nbt0) + 1)
        return ok

    def tail_grads(self, what, o, dgamma, dbeta, dy=None, side=None, dy2=None, dgamma2=None, dbeta2=None):
        """A tail backward against :func:`tail_bwd`'s ``o``: the per-channel sums (d(gamma) = sum dz xhat, d(beta) =
        sum dz; the ambiguous elements by their |term|) and the relative-L2 kinds."""
        ambg = None if o["amb"] is None else o["amb"].double() * o["gfull"].abs()
        if o["amb"] is not None:
            self.left_out(what, o["amb"])
        ok = self.sums("dbeta", what, dbeta, o["dz"], ambg)
        ok &= self.sums("dgamma", what, dgamma, o["dz"] * o["xhat"], None if ambg is None else ambg * o["xhat"].abs())
        ok &= self.l2("dgamma", what + " dgamma", dgamma, o["dgamma"])
        ok &= self.l2("dbeta", what + " dbeta", dbeta, o["dbeta"])
        if dy is not None:
            ok &= self.l2("dy", what + " dy", dy, o["dy"])
        if side is not None:
            ok &= self.l2("side", what + " side", side, o["side"])
        if dy2 is not None:
            ok &= self.l2("dy", what + " dy2", dy2, o["dy2"])
            ok &= self.sums("dgamma", what + " shortcut", dgamma2, o["dz"] * o["xhat2"],
                            None if ambg is None else ambg * o["xhat2"].abs())
            ok &= self.l2("dgamma", what + " dgamma2", dgamma2, o["dgamma2"])
            ok &= self.l2("dbeta", what + " dbeta2", dbeta2, o["dbeta2"])
        return ok

    def done(self):
        print(f"largest mask-ambiguous share of any tensor {self.share:.3e} (cap {AMB_CAP})")
        super().done()
