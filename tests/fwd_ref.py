"""Plain fp64 references and input builders of the forward path (tests/test_fwd_path_gpu.py; checked on the CPU by
tests/test_fwd_ref.py): the forward convolution with its bias and per-channel statistics, the BN constants and
running statistics, the BN forward tails and the normalise-on-load operand.  CPU torch only; nothing here imports
the extension.

The conv epilogue accumulates sum(y) and sum(y^2) from the UNROUNDED fp32 value acc + bias, not from the stored bf16
y.  With integer-valued inputs (x in [-4, 4], w in [-2, 2], bias in [-8, 8]; all exact in bf16) that value and every
partial sum of it is an integer below 2^24 in any order, so y and both statistics compare with ``==``
(tests/test_fwd_ref.py asserts sum|y| < 2^24 and sum(y^2) < 2^24 per channel for every integer case).
"""
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from wpath_ref import NAN, SENT, gen, ints

ACT_NONE, ACT_RELU, ACT_SIGMOID, SIGMUL, ADD_RELU, POOL_RELU = range(6)
GUARD_ROWS = 2            # sentinel rows of the output pitch before and after the addressed output
NOL_MARGIN = 2.0 ** -21   # relative distance from a bf16 rounding boundary below which an operand is ambiguous


def f32(x):
    """A hyperparameter as the kernel holds it: rounded to fp32, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------
# A. forward convolution
@dataclass
class FCase:
    """One forward convolution as the kernels address it.  The input is one or two channel segments (C0 + C1 = Cs),
    each a slice [off, off + C) of a buffer of pitch ld; the output a slice [ooff, ooff + Co) of a buffer of pitch
    ldo; G groups whose input buffers lie ``gap`` and whose output buffers ``ogap`` elements further apart than one
    group's buffer."""
    name: str
    B: int
    H: int
    W: int
    C0: int
    Co: int
    KH: int = 3
    KW: int = 3
    sh: int = 1
    sw: int = 1
    ph: int = 1
    pw: int = 1
    C1: int = 0
    G: int = 1
    ld0: int = 0
    off0: int = 0
    ld1: int = 0
    off1: int = 0
    gap: int = 0
    ldo: int = 0
    ooff: int = 0
    ogap: int = 0
    bias: bool = True
    real: bool = False       # randn data rounded to bf16 instead of integers
    wlim: int = 2            # integer weights in [-wlim, wlim]
    seed: int = 0
    Ho: int = field(init=False)
    Wo: int = field(init=False)

    def __post_init__(self):
        self.ld0 = self.ld0 or self.C0
        self.ld1 = self.ld1 or self.C1
        self.ldo = self.ldo or self.Co
        self.Ho = (self.H + 2 * self.ph - self.KH) // self.sh + 1
        self.Wo = (self.W + 2 * self.pw - self.KW) // self.sw + 1

    @property
    def Cs(self):
        return self.C0 + self.C1

    @property
    def M(self):
        return self.B * self.Ho * self.Wo

    @property
    def K(self):
        return self.KH * self.KW * self.Cs


def in_view(buf, c: FCase, seg=0):
    """The [G, B, H, W, C] slice a conv reads of segment ``seg``'s flat buffer [G, pixels * ld + gap] (any device)."""
    ld, off, C = (c.ld1, c.off1, c.C1) if seg else (c.ld0, c.off0, c.C0)
    P = c.B * c.H * c.W
    return buf[:, :P * ld].view(c.G, c.B, c.H, c.W, ld)[..., off:off + C]


def in_buf(vals, c, seg=0):
    """``vals`` [G, B, H, W, C] as segment ``seg``'s flat bf16 buffer, NaN outside the addressed slice.  Like the
    views above and the output builders below it takes any record with the fields it names (tests/dgrad_ref.py
    addresses a dgrad's dy and dx through them)."""
    ld = c.ld1 if seg else c.ld0
    P = c.B * c.H * c.W
    buf = torch.full((c.G, P * ld + c.gap), NAN)
    in_view(buf, c, seg).copy_(vals)
    return buf.bfloat16()


def out_buf(c: FCase):
    """The flat bf16 output buffer, SENT everywhere: GUARD_ROWS rows, G groups of (pixels * ldo + ogap), GUARD_ROWS
    rows."""
    return torch.full((2 * GUARD_ROWS * c.ldo + c.G * (c.M * c.ldo + c.ogap),), SENT).bfloat16()


def out_view(flat, c: FCase):
    """The [G, B, Ho, Wo, Co] slice of :func:`out_buf` (any device) the conv writes."""
    body = flat[GUARD_ROWS * c.ldo:flat.numel() - GUARD_ROWS * c.ldo].view(c.G, c.M * c.ldo + c.ogap)
    return body[:, :c.M * c.ldo].view(c.G, c.B, c.Ho, c.Wo, c.ldo)[..., c.ooff:c.ooff + c.Co]


def out_foreign(flat, c: FCase):
    """Every element of the flat output buffer outside the addressed slice (a 1-D copy): must still be SENT."""
    mask = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    out_view(mask, c).fill_(False)
    return flat[mask]


def conv_inputs(c: FCase) -> dict:
    """bf16 buffers as the kernel reads them (``buf0``, ``buf1``: [G, pixels * pitch + gap], NaN outside the
    addressed slices), fp32 weights ``w`` [G, Co, Cs, KH, KW] and bias ``b`` [G, Co] (None without bias) holding
    bf16-exact values, and the operand ``x`` [G, B, H, W, Cs] in fp64."""
    g = gen(5000 + c.seed)
    if c.real:
        x = torch.randn(c.G, c.B, c.H, c.W, c.Cs, generator=g).bfloat16().float()
        w = (torch.randn(c.G, c.Co, c.Cs, c.KH, c.KW, generator=g) / c.K ** 0.5).bfloat16().float()
        b = torch.randn(c.G, c.Co, generator=g)
    else:
        x = ints(g, (c.G, c.B, c.H, c.W, c.Cs), 4)
        w = ints(g, (c.G, c.Co, c.Cs, c.KH, c.KW), c.wlim, 0.375 if c.wlim > 1 else 0.25)
        b = ints(g, (c.G, c.Co), 8, 0.0)
    return {"buf0": in_buf(x[..., :c.C0], c, 0), "buf1": in_buf(x[..., c.C0:], c, 1) if c.C1 else None,
            "w": w, "b": b if c.bias else None, "x": x.double()}


def conv2d_nhwc(x, w, b, c: FCase, pad_value=None, skip=None):
    """fp64 conv of one group, tap by tap: x [B, H, W, Cs], w [Co, Cs, KH, KW], b [Co] or None -> [B, Ho, Wo, Co].
    ``pad_value`` [Cs]: what the padding holds instead of zero; ``skip`` = (kh, kw, oh): that tap is left out of
    output row ``oh`` (both only for the sensitivity tests' wrong references)."""
    x, w = x.double(), w.double()
    xp = F.pad(x, (0, 0, c.pw, c.pw, c.ph, c.ph))
    if pad_value is not None:
        xp = pad_value.double().expand_as(xp).clone()
        xp[:, c.ph:c.ph + c.H, c.pw:c.pw + c.W] = x
    y = torch.zeros(c.B, c.Ho, c.Wo, c.Co, dtype=torch.float64, device=x.device)
    for kh in range(c.KH):
        for kw in range(c.KW):
            win = xp[:, kh:kh + (c.Ho - 1) * c.sh + 1:c.sh, kw:kw + (c.Wo - 1) * c.sw + 1:c.sw]
            t = win @ w[:, :, kh, kw].t()
            if skip is not None and skip[:2] == (kh, kw):
                t[:, skip[2]] = 0
            y += t
    return y if b is None else y + b.double()


def conv_fwd(c: FCase, inp: dict) -> dict:
    """``y`` [G, B, Ho, Wo, Co]: the exact fp64 output; ``ybf``: its bf16 round-to-nearest-even image; ``s1``, ``s2``
    [G, Co]: sum(y) and sum(y^2) of the UNROUNDED y per group and channel; ``T`` = conv(|x|, |w|) + |b|."""
    ys, Ts = [], []
    for z in range(c.G):
        b = None if inp["b"] is None else inp["b"][z]
        ys.append(conv2d_nhwc(inp["x"][z], inp["w"][z], b, c))
        Ts.append(conv2d_nhwc(inp["x"][z].abs(), inp["w"][z].abs(), None if b is None else b.abs(), c))
    y = torch.stack(ys)
    return {"y": y, "ybf": y.float().bfloat16(), "s1": y.sum((1, 2, 3)), "s2": (y * y).sum((1, 2, 3)),
            "T": torch.stack(Ts)}


def randn_stat_bounds(c: FCase, ref: dict):
    """Per-channel bounds [G, Co] of the statistics of a real-valued case: with n pixels per channel, K products per
    output, T = conv(|x|, |w|) + |b| and delta = K 2^-24 T (the worst case of an fp32 accumulation of K products),
      |d sum(y)|   <= sum(delta) + n 2^-24 sum|ref|
      |d sum(y^2)| <= sum(2 |ref| delta + delta^2) + (n + 1) 2^-24 sum(ref^2)."""
    u, n = 2.0 ** -24, c.M
    y, d = ref["y"], c.K * 2.0 ** -24 * ref["T"]
    red = (1, 2, 3)
    return (d.sum(red) + n * u * y.abs().sum(red),
            (2 * y.abs() * d + d * d).sum(red) + (n + 1) * u * (y * y).sum(red))


# ---------------------------------------------------------------------------------------------------
# B. BN constants, running statistics, tails
def bn_consts(stats, count, gamma, beta, eps):
    """[..., 4, C] fp64 (scale, shift, mean, invstd) of a training-mode BN from the totals ``stats`` [..., 2, C]
    (sum(y), sum(y^2)) over ``count`` elements per channel; also returns the biased variance."""
    s, ss = stats.double().unbind(-2)
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * inv
    return torch.stack([scale, beta.double() - mean * scale, mean, inv], -2), var


def eval_consts(run_mean, run_var, gamma, beta, eps):
    """[..., 4, C] fp64 constants of an eval-mode BN (running statistics)."""
    inv = 1.0 / torch.sqrt(run_var.double() + eps)
    scale = gamma.double() * inv
    return torch.stack([scale, beta.double() - run_mean.double() * scale, run_mean.double(), inv], -2)


def running(rm0, rv0, mean, var, count, momentum):
    """fp64 running statistics after one training step: the unbiased variance enters (``count == 1`` keeps the biased
    one, as csrc/common.h bn_channel does)."""
    unb = var * count / (count - 1) if count > 1 else var
    return (1.0 - momentum) * rm0.double() + momentum * mean, (1.0 - momentum) * rv0.double() + momentum * unb


def pool2x2_ceil(t):
    """2x2 / stride-2 ceil-mode max over NHWC ``t`` [..., H, W, C] (partial windows at odd H / W)."""
    H, W, C = t.shape[-3:]
    lead = t.shape[:-3]
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    tp = torch.full(lead + (2 * Hp, 2 * Wp, C), float("-inf"), dtype=t.dtype, device=t.device)
    tp[..., :H, :W, :] = t
    return tp.view(lead + (Hp, 2, Wp, 2, C)).amax((-2, -4))


def tail_fwd(kind, y, consts, r=None, consts2=None):
    """The unrounded fp64 output of the forward tail ``kind`` on NHWC ``y`` with the BN constants ``consts`` [4, C]
    (rows scale, shift); ``r``: SIGMUL's multiplier / ADD_RELU's residual, ``consts2``: the residual's own BN
    (projection shortcut).  POOL_RELU: the 2x2 ceil-mode max of relu(BN(y))."""
    k = consts.double()
    t = y.double() * k[..., 0, :] + k[..., 1, :]
    if kind == ACT_NONE:
        return t
    if kind == ACT_RELU:
        return t.clamp_min(0)
    if kind == ACT_SIGMOID:
        return torch.sigmoid(t)
    if kind == SIGMUL:
        return torch.sigmoid(t) * r.double()
    if kind == ADD_RELU:
        rr = r.double()
        if consts2 is not None:
            k2 = consts2.double()
            rr = rr * k2[..., 0, :] + k2[..., 1, :]
        return (t + rr).clamp_min(0)
    if kind == POOL_RELU:
        return pool2x2_ceil(t.clamp_min(0))
    raise ValueError(kind)


def ulp_bf16(a):
    """The spacing of bf16 above |a| (fp64; 0 at 0)."""
    _, e = torch.frexp(a.double().abs())
    return torch.where(a == 0, torch.zeros_like(a, dtype=torch.float64), torch.ldexp(torch.ones_like(a, dtype=torch.float64), e - 8))


def bf16_rne(v):
    """fp64 -> the nearest bf16 value (ties to even) in ONE rounding, returned in fp64 (normal range)."""
    u = ulp_bf16(v).clamp_min(1e-300)
    return torch.round(v.double() / u) * u


def nol_operand(y, scale, shift, kind, margin=NOL_MARGIN, slack=0.0):
    """(a, amb): the normalise-on-load operand bf16(act(y * scale + shift)) in fp64 -- the padding around it is zero,
    not BN(0): pad ``a`` itself -- and the map of AMBIGUOUS elements, whose fp64 value lies within ``margin``
    (relative; plus ``slack`` absolute, for constants the kernel did not publish) of a bf16 rounding boundary: a
    fused or an unfused fp32 evaluation may land on either neighbour."""
    v = y.double() * scale.double() + shift.double()
    if kind == ACT_RELU:
        v = v.clamp_min(0)
    a = bf16_rne(v)
    mag = torch.where(v.abs() >= a.abs(), a.abs() + ulp_bf16(a), a.abs() - _ulp_below(a))  # the neighbour on v's side
    mid = 0.5 * (a + torch.sign(v) * mag)
    amb = ((v - mid).abs() <= margin * v.abs() + slack) & (v != 0)
    return a, amb


def _ulp_below(a):
    """The spacing of bf16 towards zero from |a| (half of ulp_bf16 at a power of two)."""
    u = ulp_bf16(a)
    m, _ = torch.frexp(a.double().abs())
    return torch.where(m == 0.5, u / 2, u)


def nol_conv(a, amb, w, c: FCase):
    """The fp64 conv of the (zero-padded) operand ``a`` [B, H, W, Cs] with ``w`` [Co, Cs, KH, KW] and the per-element
    slack the ambiguous operands may cost: sum over the receptive field of |w| ulp_bf16(a)."""
    return conv2d_nhwc(a, w, None, c), conv2d_nhwc(amb.double() * ulp_bf16(a), w.abs(), None, c)


def one_ulp(ref):
    """The project's one-bf16-ulp bound of a stored activation: 2^-8 |ref| + 1e-5 max|ref|."""
    return ref.abs() * 2.0 ** -8 + 1e-5 * ref.abs().max()


def tail_y(seed, shape, C, G=1):
    """bf16 y ~ 2 N(0,1) + 0.3 and r ~ N(0,1) [G, B, H, W, C] and fp32 BN parameters / state [G, C] of a forward-tail
    case: gamma in [0.5, 1.5], beta ~ 0.1 N(0,1), non-trivial running statistics; the same for the residual's BN
    (suffix 2; y2 ~ N(0,1) + 1)."""
    g = gen(7000 + seed)
    s = (G,) + tuple(shape) + (C,)
    d = {"y": (2 * torch.randn(s, generator=g) + 0.3).bfloat16(), "r": torch.randn(s, generator=g).bfloat16(),
         "y2": (torch.randn(s, generator=g) + 1).bfloat16()}
    for sfx in ("", "2"):
        d["gamma" + sfx] = torch.rand(G, C, generator=g) + 0.5
        d["beta" + sfx] = 0.1 * torch.randn(G, C, generator=g)
        d["rm" + sfx] = 0.5 * torch.randn(G, C, generator=g)
        d["rv" + sfx] = 0.5 + torch.rand(G, C, generator=g)
    for _ in range(8):  # move y off every ReLU decision (the statistics move with it: repeat until none is left)
        close = relu_arguments_close(d, TAIL_MARGIN)
        if not bool(close.any()):
            break
        d["y"] = torch.where(close, d["y"] + 0.25, d["y"])
    return d


TAIL_MARGIN = 1e-5  # bwd_ref.JOIN_MARGIN: no ReLU argument of the tail inputs is closer to zero


def tail_consts(d, eps=1e-5):
    """fp32-rounded batch constants [G, 4, C] of y and of y2 of :func:`tail_y`."""
    n = d["y"][0].numel() // d["y"].shape[-1]
    k, _ = bn_consts(totals(d["y"]), n, d["gamma"], d["beta"], eps)
    k2, _ = bn_consts(totals(d["y2"]), n, d["gamma2"], d["beta2"], eps)
    return k.float(), k2.float()


def relu_arguments_close(d, margin):
    """Elements of :func:`tail_y` whose ACT_RELU / POOL_RELU argument BN(y), identity ADD_RELU argument BN(y) + r or
    projection ADD_RELU argument BN(y) + BN2(y2) lies within ``margin`` of zero."""
    k, k2 = tail_consts(d)
    k, k2 = k.double()[:, :, None, None, None], k2.double()[:, :, None, None, None]
    t = d["y"].double() * k[:, 0] + k[:, 1]
    t2 = d["y2"].double() * k2[:, 0] + k2[:, 1]
    return (t.abs() < margin) | ((t + d["r"].double()).abs() < margin) | ((t + t2).abs() < margin)


def nol_inputs(c: FCase, big_shift=False) -> dict:
    """A normalise-on-load conv: the previous conv's pre-BN ``y`` [G, B, H, W, Cs] (bf16, ~ 2 N(0,1) + 0.3; ``buf0``
    as the kernel reads it, NaN outside the slice), that BN's parameters and state [G, Cs] and bf16-exact weights
    ``w`` [G, Co, Cs, KH, KW].  ``big_shift``: |beta| ~ 3, so that BN(0) = shift in the padding would be far off."""
    g = gen(9000 + c.seed)
    y = (2 * torch.randn(c.G, c.B, c.H, c.W, c.Cs, generator=g) + 0.3).bfloat16()
    d = {"y": y, "buf0": in_buf(y.float(), c, 0),
         "gamma": torch.rand(c.G, c.Cs, generator=g) + 0.5, "beta": 0.1 * torch.randn(c.G, c.Cs, generator=g),
         "rm": 0.5 * torch.randn(c.G, c.Cs, generator=g), "rv": 0.5 + torch.rand(c.G, c.Cs, generator=g),
         "w": (torch.randn(c.G, c.Co, c.Cs, c.KH, c.KW, generator=g) / c.K ** 0.5).bfloat16().float()}
    if big_shift:
        sign = torch.randint(0, 2, (c.G, c.Cs), generator=g).float() * 2 - 1
        d["beta"] = sign * (3.0 + 0.2 * torch.rand(c.G, c.Cs, generator=g))
    return d




def totals(y):
    """fp64 [G, 2, C] (sum(y), sum(y^2)) of [G, B, H, W, C]."""
    y = y.double()
    return torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1)


def spread(tot, nrep, NREP, seed, fill=0.0):
    """Totals [G, 2, C] spread over the first ``nrep`` of NREP replica rows [G, NREP, 2, C] (fp64; the rows sum to
    the totals up to fp64 rounding); rows >= nrep hold ``fill``."""
    g = gen(8000 + seed)
    G, _, C = tot.shape
    wgt = torch.rand(G, nrep, 1, 1, generator=g, dtype=torch.float64) + 0.1
    wgt = wgt / wgt.sum(1, keepdim=True)
    rep = torch.full((G, NREP, 2, C), float(fill), dtype=torch.float64)
    rep[:, :nrep] = tot.unsqueeze(1) * wgt
    return rep


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_fwd_path_gpu.py part A
BASE, DEEP = (2, 17, 42), (2, 9, 21)


def _c(name, shape, C0, Co, **kw):
    return FCase(name, *shape, C0, Co, **kw)


FCASES = [
    _c("3x3 p1", BASE, 32, 48, seed=1),
    _c("3x3 s2", BASE, 64, 48, sh=2, sw=2, seed=2),
    _c("1x1 s2", BASE, 256, 48, KH=1, KW=1, sh=2, sw=2, ph=0, pw=0, seed=3),
    _c("5x5 p2", DEEP, 48, 48, KH=5, KW=5, ph=2, pw=2, wlim=1, seed=4),
    _c("1x7", DEEP, 32, 48, KH=1, KW=7, ph=0, pw=3, seed=5),
    _c("7x1", DEEP, 32, 48, KH=7, KW=1, ph=3, pw=0, seed=6),
    _c("3x3 p0", BASE, 32, 48, ph=0, pw=0, seed=7),
    _c("two segments", BASE, 16, 48, C1=16, ld0=24, off0=8, ld1=40, off1=16, seed=8),
    _c("G3 gaps", DEEP, 32, 48, G=3, ld0=40, off0=8, gap=16, ogap=8, seed=9),
    _c("out slice", BASE, 32, 48, ldo=64, ooff=8, seed=10),
    _c("no bias", BASE, 32, 48, bias=False, seed=11),
    _c("3x3 Cs16 Co32", DEEP, 16, 32, seed=12),            # the patch kernels' 16-channel slice alone
]
RCASES = [
    _c("real 3x3", BASE, 32, 48, real=True, seed=21),
    _c("real 1x1", BASE, 64, 48, KH=1, KW=1, ph=0, pw=0, real=True, seed=22),
]
NCASES = [
    _c("nol 3x3", BASE, 32, 48, real=True, bias=False, seed=31),
    _c("nol 3x3 G2", DEEP, 32, 48, G=2, ld0=40, off0=8, gap=8, real=True, bias=False, seed=32),
    _c("nol big shift", DEEP, 32, 48, real=True, bias=False, seed=33),
    _c("nol 1x1", DEEP, 64, 48, KH=1, KW=1, ph=0, pw=0, real=True, bias=False, seed=34),
]
FCASE = {c.name: c for c in FCASES + RCASES + NCASES}


# ---------------------------------------------------------------------------------------------------
class Checker:
    """Collects every violated bound, naming the first offending element, and the worst observed value of each kind
    of toleranced assertion (exact kinds count their comparisons instead)."""

    def __init__(self):
        self.worst, self.bad, self.count = {}, [], {}

    def _note(self, kind, v):
        self.worst[kind] = max(self.worst.get(kind, 0.0), v)

    @staticmethod
    def _where(mask):
        i = int(mask.reshape(-1).int().argmax())
        return tuple(int(j) for j in torch.unravel_index(torch.tensor(i), mask.shape))

    def exact(self, what, got, ref):
        """Equal after a cast to fp64 (a NaN on either side is a mismatch)."""
        self.count["exact"] = self.count.get("exact", 0) + 1
        if tuple(got.shape) != tuple(ref.shape):
            self.bad.append((what, "shape", tuple(got.shape), tuple(ref.shape)))
            return False
        g, r = got.double(), ref.double().to(got.device)
        ne = ~(g == r)
        if bool(ne.any()):
            at = self._where(ne)
            self.bad.append((what, "exact", f"{int(ne.sum())} elements differ, first at {at}: got {g[at].item()!r} "
                             f"ref {r[at].item()!r}"))
            return False
        return True

    def bits(self, what, got, ref):
        """Two tensors of one dtype bit for bit (bf16, fp32, fp64 or int64)."""
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        if got.dtype != ref.dtype:
            self.bad.append((what, "dtype", got.dtype, ref.dtype))
            return False
        return self.exact(what, got.contiguous().view(it), ref.to(got.device).contiguous().view(it))

    def bounded(self, kind, what, got, ref, bound):
        """|got - ref| <= bound per element (fp64); records max err / bound.  A non-finite ``got`` is out of bound."""
        ref, bound = ref.to(got.device), bound.to(got.device)
        err = (got.double() - ref).abs()
        ok = err <= bound
        ratio = err / bound.clamp_min(1e-300)
        fin = torch.isfinite(ratio)
        self._note(kind + " err / bound", float(ratio[fin].max()) if bool(fin.any()) else 0.0)
        if not bool(ok.all()):
            at = self._where(~ok)
            self.bad.append((what, kind, f"{int((~ok).sum())} elements out of bound, first at {at}: got "
                             f"{got[at].item()!r} ref {ref[at].item()!r} bound {bound[at].item():.3e}"))
            return False
        return True

    def sentinels(self, what, t, value=SENT):
        """Every element of ``t`` still holds ``value``."""
        self.count["sentinel"] = self.count.get("sentinel", 0) + 1
        ne = ~(t.double() == value)
        if bool(ne.any()):
            at = self._where(ne)
            self.bad.append((what, "sentinel", f"{int(ne.sum())} elements written, first at {at}: {t[at].item()!r}"))
            return False
        return True

    def true(self, what, cond):
        if not cond:
            self.bad.append((what, "condition"))
        return bool(cond)

    # --- the composite checks of tests/test_fwd_path_gpu.py (run against perturbed references on the CPU) ---
    def conv_exact(self, what, c, flat, stats, ref, nrep=None):
        """An integer conv launch: y == bf16(ref) bit for bit, the replica rows sum to the exact statistics (rows >=
        ``nrep`` zero), the output finite (no poisoned column read), every sentinel intact.  ``flat``: the output
        buffer after the launch, ``stats`` [G, NREP, 2, Co] or None."""
        y = out_view(flat, c)
        ok = self.true(what + " finite", bool(torch.isfinite(y.float()).all()))
        ok &= self.bits(what + " y", y.contiguous(), ref["ybf"])
        ok &= self.sentinels(what + " output sentinels", out_foreign(flat, c))
        if stats is not None:
            ok &= self.stat_totals(what, stats, ref, nrep)
        return ok

    def stat_totals(self, what, stats, ref, nrep=None):
        ok = self.exact(what + " sum(y)", stats[:, :, 0].sum(1), ref["s1"])
        ok &= self.exact(what + " sum(y^2)", stats[:, :, 1].sum(1), ref["s2"])
        if nrep is not None:
            ok &= self.true(what + f" replica rows >= {nrep} zero", bool((stats[:, nrep:] == 0).all()))
        return ok

    def consts(self, what, got, ref, beta, extra=None):
        """Published constants [..., 4, C] against bn_consts: mean 2^-24 |mean|, invstd 4 2^-24 relative, scale
        5 2^-24 relative, shift 8 2^-24 (|beta| + |mean scale|).  ``extra`` [..., 4, C] (rows as the constants):
        what totals that are not exact may add to each (tests/layer_ref.py stat_slack)."""
        u = 2.0 ** -24
        r = ref.to(got.device)
        sc, sh, mu, inv = r.unbind(-2)
        x = torch.zeros_like(r) if extra is None else extra.to(got.device)
        ok = self.bounded("mean", what, got[..., 2, :], mu, u * mu.abs() + x[..., 2, :])
        ok &= self.bounded("invstd", what, got[..., 3, :], inv, 4 * u * inv.abs() + x[..., 3, :])
        ok &= self.bounded("scale", what, got[..., 0, :], sc, 5 * u * sc.abs() + x[..., 0, :])
        ok &= self.bounded("shift", what, got[..., 1, :], sh,
                           8 * u * (beta.double().to(got.device).abs() + (mu * sc).abs()) + x[..., 1, :])
        return ok

    def running_stats(self, what, rm, rv, rm0, rv0, mean, var, count, momentum, extra=(0.0, 0.0)):
        """Running statistics after one step: |err| <= 4 2^-24 (|(1 - m) old| + |m new|), m the fp32 momentum;
        ``extra`` = (mean, biased variance) slack of totals that are not exact."""
        m, u = f32(momentum), 2.0 ** -24
        unb = var * count / (count - 1) if count > 1 else var
        ref_m, ref_v = running(rm0, rv0, mean, var, count, m)
        xv = extra[1] * count / (count - 1) if count > 1 else extra[1]
        ok = self.bounded("run_mean", what, rm, ref_m,
                          4 * u * (((1 - m) * rm0.double()).abs() + (m * mean).abs()) + m * extra[0])
        ok &= self.bounded("run_var", what, rv, ref_v,
                           4 * u * (((1 - m) * rv0.double()).abs() + (m * unb).abs()) + m * xv)
        return ok

    def act(self, what, got, ref, extra=None, kind="act"):
        """A stored bf16 activation within one ulp of the fp64 reference (+ ``extra`` per element)."""
        b = one_ulp(ref)
        return self.bounded(kind, what, got, ref, b if extra is None else b + extra)

    def done(self):
        print("worst observed", {k: f"{v:.3g}" for k, v in self.worst.items()}, "exact comparisons", self.count)
        assert not self.bad, self.bad[:20]
