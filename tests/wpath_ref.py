"""Plain fp64 references and input builders of the weight path (tests/test_wpath_gpu.py; checked on the CPU by
tests/test_wpath_ref.py): weight gradient of a convolution in the slab's column order, the finalize's sum over
splits, Adam with coupled L2, the packed-tap stem input.  CPU torch only; nothing here imports the extension.

Integer-valued inputs make every sum of products exact in fp32 in any order: x and dy are integers in [-4, 4]
(exact in bf16), a normalise-on-load operand is at most 11, so a weight-gradient element is at most
44 * 1428 < 2^16 in magnitude and every partial sum of it is an integer below 2^24.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F

NAN = float("nan")
SENT = -12288.0          # what a kernel must not write (exact in fp32, bf16 and int64)
MAX_PX = 1428            # (2, 17, 42): the largest output map of any case
ACT_NONE, ACT_RELU = 0, 1


def pad_to(x, m):
    return (x + m - 1) // m * m


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lim=4, zero=0.16):
    """Integers in [-lim, lim] (fp32), about a quarter of them zero at lim = 4."""
    v = torch.randint(-lim, lim + 1, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) >= zero)


# ---------------------------------------------------------------------------------------------------
# A. weight gradient
@dataclass
class WCase:
    """One convolution's weight-gradient problem as the kernels address it.  The input is one or two channel
    segments (C0 + C1 = Cs), each a slice [off, off + C) of a buffer of pitch ld; dy a slice [doff, doff + Co) of a
    buffer of pitch ldd; G groups ``gap`` elements further apart than one group's buffer."""
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
    ldd: int = 0
    doff: int = 0
    gap: int = 0
    nol: Optional[int] = None   # normalise-on-load activation kind
    real: bool = False          # randn inputs rounded to bf16 instead of integers
    seed: int = 0
    Ho: int = field(init=False)
    Wo: int = field(init=False)

    def __post_init__(self):
        self.ld0 = self.ld0 or self.C0
        self.ld1 = self.ld1 or self.C1
        self.ldd = self.ldd or self.Co
        self.Ho = (self.H + 2 * self.ph - self.KH) // self.sh + 1
        self.Wo = (self.W + 2 * self.pw - self.KW) // self.sw + 1

    @property
    def Cs(self):
        return self.C0 + self.C1

    @property
    def taps(self):
        return self.KH * self.KW

    @property
    def M(self):
        return self.B * self.Ho * self.Wo

    @property
    def Npad(self):
        return pad_to(self.Co, 16)

    @property
    def Kpad(self):
        return pad_to(self.taps * self.Cs, 64)


def _sliced(vals, ld, off, gap):
    """``vals`` [G, P, C] as the slice [off, off + C) of a [G, P * ld + gap] buffer whose other elements are NaN."""
    G, P, C = vals.shape
    buf = torch.full((G, P * ld + gap), NAN)
    buf[:, :P * ld].view(G, P, ld)[:, :, off:off + C] = vals
    return buf.bfloat16()


def wgrad_inputs(c: WCase) -> dict:
    """bf16 buffers as the kernel reads them (``buf0``, ``buf1``, ``dybuf``: [G, pixels * pitch + gap], NaN outside
    the addressed slices), the normalise-on-load constants ``consts`` [G, 4, Cs] (scale, shift; the mean / invstd
    rows NaN: the weight gradient must not read them), and the operands in fp64: ``x`` [G, B, H, W, Cs] (after
    normalise-on-load), ``dy`` [G, B, Ho, Wo, Co]."""
    g = gen(1000 + c.seed)
    Pi, Po = c.B * c.H * c.W, c.M
    if c.real:
        raw = torch.randn(c.G, Pi, c.Cs, generator=g).bfloat16().float()
        dy = torch.randn(c.G, Po, c.Co, generator=g).bfloat16().float()
    else:
        raw = ints(g, (c.G, Pi, c.Cs))
        dy = ints(g, (c.G, Po, c.Co))
    out = {"buf0": _sliced(raw[..., :c.C0], c.ld0, c.off0, c.gap), "dybuf": _sliced(dy, c.ldd, c.doff, c.gap),
           "buf1": _sliced(raw[..., c.C0:], c.ld1, c.off1, c.gap) if c.C1 else None, "consts": None}
    x = raw.double()
    if c.nol is not None:
        k = torch.full((c.G, 4, c.Cs), NAN)
        k[:, 0] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.G, c.Cs), generator=g)]
        k[:, 1] = torch.randint(-3, 4, (c.G, c.Cs), generator=g).float()
        out["consts"] = k
        x = nol_operand(raw, k, c.nol, torch.float64)
        out["x32"] = nol_operand(raw, k, c.nol, torch.float32)
    out["x"] = x.view(c.G, c.B, c.H, c.W, c.Cs)
    out["dy"] = dy.double().view(c.G, c.B, c.Ho, c.Wo, c.Co)
    return out


def nol_operand(raw, consts, kind, dtype):
    """bf16(act(x * scale + shift)) evaluated in ``dtype``, returned in ``dtype``: raw [G, P, Cs], consts [G, 4, Cs]."""
    v = raw.to(dtype) * consts[:, 0:1].to(dtype) + consts[:, 1:2].to(dtype)
    if kind == ACT_RELU:
        v = v.clamp_min(0)
    return v.float().bfloat16().to(dtype)


def wgrad_cols(x, c):
    """The im2col operand [B, Cs, taps, Ho, Wo] of x [B, H, W, Cs] (zero padding; an explicit Ho / Wo below the
    geometry's own, as of the packed-tap stem, keeps the leading rows / columns)."""
    cols = F.unfold(x.permute(0, 3, 1, 2), (c.KH, c.KW), padding=(c.ph, c.pw), stride=(c.sh, c.sw))
    Hn = (c.H + 2 * c.ph - c.KH) // c.sh + 1
    Wn = (c.W + 2 * c.pw - c.KW) // c.sw + 1
    return cols.view(c.B, c.Cs, c.taps, Hn, Wn)[..., :c.Ho, :c.Wo]


def wgrad_from_cols(cols, dy, pix=None):
    """[Co, taps, Cs] (the slab's order: column k = tap * Cs + ci) from wgrad_cols and dy [B, Ho, Wo, Co]; ``pix``
    [B, Ho, Wo] bool restricts the sum to those output pixels."""
    if pix is not None:
        dy = dy * pix.unsqueeze(-1)
    return torch.einsum("bcthw,bhwo->otc", cols, dy)


def wgrad_ref(x, dy, c, pix=None):
    """fp64 weight gradient of one group in the slab's order [Co, taps, Cs]: x [B, H, W, Cs], dy [B, Ho, Wo, Co]."""
    return wgrad_from_cols(wgrad_cols(x, c), dy, pix)


def to_nchw(slab_order, c):
    """[Co, taps, Cs] -> the reference weight layout [Co, Cs, KH, KW]."""
    return slab_order.permute(0, 2, 1).reshape(c.Co, c.Cs, c.KH, c.KW)


def split_pixels(c, splits, mps, strip_rows=0):
    """[splits, B, Ho, Wo] bool: the output pixels of each split.  Im2col kernels: flattened pixels
    [s * mps, (s + 1) * mps); patch kernels (``strip_rows`` = R): units (image, strip of R rows) [s * mps, ...)."""
    if strip_rows:
        nstrip = math.ceil(c.Ho / strip_rows)
        unit = (torch.arange(c.B).view(-1, 1, 1) * nstrip + (torch.arange(c.Ho) // strip_rows).view(1, -1, 1))
        unit = unit.expand(c.B, c.Ho, c.Wo)
    else:
        unit = torch.arange(c.M).view(c.B, c.Ho, c.Wo)
    return torch.stack([(unit >= s * mps) & (unit < (s + 1) * mps) for s in range(splits)])


def forced_plans(M, MCH):
    """Two (splits, m_per_split) plans of an im2col config: the last split shorter than one chunk (M is no multiple
    of MCH: the smallest whole-chunk m_per_split whose remainder is M % MCH, at most 8 splits); one split."""
    q = M // MCH
    assert M % MCH and q >= 1, (M, MCH)
    d = next(d for d in range(math.ceil(q / 7), q + 1) if q % d == 0)
    return (q // d + 1, d * MCH), (1, pad_to(M, MCH))


# --- the cases of tests/test_wpath_gpu.py (part A) ---
BASE, DEEP, WIDE1, WIDE2 = (2, 17, 42), (2, 9, 21), (1, 6, 122), (2, 5, 84)


def _c(name, shape, C0, Co, **kw):
    return WCase(name, *shape, C0, Co, **kw)


# per-conv launches: every config valid for the case runs it under the engine's plan and the two forced plans
WCASES = [
    _c("3x3 p1", BASE, 16, 16, seed=1),
    _c("3x3 p0 Cs8 Co8", BASE, 8, 8, ph=0, pw=0, seed=2),
    _c("3x3 s2 odd Co24", (2, 17, 43), 16, 24, sh=2, sw=2, seed=3),
    _c("1x1 s2 Co40", BASE, 64, 40, KH=1, KW=1, sh=2, sw=2, ph=0, pw=0, seed=4),
    _c("1x7", DEEP, 16, 16, KH=1, KW=7, ph=0, pw=3, seed=5),
    _c("7x1", DEEP, 16, 32, KH=7, KW=1, ph=3, pw=0, seed=6),
    _c("5x5 Cs8", DEEP, 8, 16, KH=5, KW=5, ph=2, pw=2, seed=7),
    _c("3x3 Co72 Kpad320", DEEP, 32, 72, seed=8),          # above a 64-row tile; Kpad 320 = 2.5 x TK 128
    _c("3x3 Co136 Cs8", DEEP, 8, 136, seed=17),            # above a 128-row tile
    _c("G2 pitched", BASE, 32, 16, G=2, ld0=48, off0=8, ldd=40, doff=16, gap=24, seed=9),
    _c("two segments", BASE, 32, 16, C1=16, ld0=40, off0=8, ld1=16, seed=10),
    _c("G2 nol relu", BASE, 32, 24, G=2, gap=8, nol=ACT_RELU, ldd=32, doff=8, seed=11),
    _c("nol none p0", DEEP, 16, 16, ph=0, pw=0, nol=ACT_NONE, seed=12),
    _c("wide row", WIDE1, 32, 32, seed=13),                # patch configs 16-19
    _c("wide row G2 two segments", WIDE2, 16, 16, C1=16, G=2, gap=16, ld0=24, off0=8, seed=14),  # patch configs 12-13
    _c("real 3x3", BASE, 16, 16, real=True, seed=15),
    _c("real 1x7 two segments", DEEP, 16, 24, C1=8, KH=1, KW=7, ph=0, pw=3, real=True, seed=16),
]
# batched launches: per config, one table of the pool's jobs that the config takes
WBATCH_IM2COL = [
    _c("b 3x3", DEEP, 16, 16, seed=21),
    _c("b G2", DEEP, 16, 24, G=2, gap=8, ld0=24, off0=8, sh=2, sw=2, seed=22),
    _c("b two segments", BASE, 8, 16, C1=8, ld0=16, seed=23),
    _c("b nol", (2, 9, 22), 16, 8, nol=ACT_RELU, ph=0, pw=0, seed=24),
    _c("b 1x1", BASE, 64, 40, KH=1, KW=1, ph=0, pw=0, ldd=48, doff=8, seed=25),
    _c("b 1x7 G2", DEEP, 16, 16, KH=1, KW=7, ph=0, pw=3, G=2, gap=8, seed=26),        # Kpad 128 (config 9)
    _c("b Cs8 nol", DEEP, 8, 24, nol=ACT_NONE, seed=27),                               # Kpad 128
    _c("b Kpad320", DEEP, 32, 72, seed=28),                                            # Kpad 320 (config 11)
    _c("b Kpad320 two segments", (2, 9, 22), 16, 16, C1=16, ld1=24, off1=8, seed=29),  # Kpad 320
]
WBATCH_PATCH = [
    _c("pb 3x3", DEEP, 32, 16, seed=31),
    _c("pb G2", DEEP, 32, 24, G=2, gap=8, ld0=40, off0=8, seed=32),
    _c("pb two segments", (2, 9, 20), 32, 16, C1=32, ld0=48, seed=33),
    _c("pb nol p0", (2, 9, 22), 32, 72, nol=ACT_RELU, ph=0, pw=0, seed=34),
    _c("pb wide", WIDE1, 32, 32, seed=35),                                             # rows of 128: configs 16-19
    _c("pb wide G2", (2, 5, 42), 32, 16, G=2, gap=16, ldd=24, doff=8, seed=36),
    _c("pb wide two segments", (2, 5, 44), 32, 16, C1=32, ld0=40, off0=8, seed=37),
    _c("pb wide nol p0", (2, 5, 46), 32, 24, nol=ACT_NONE, ph=0, pw=0, seed=38),
]


# ---------------------------------------------------------------------------------------------------
# B. finalize
FIN_SPLITS = [1, 2, 3, 8, 9, 16, 17, 33, 64, 65, 129]
# (name, G, Co, Ci, Cs, KH, KW) or a fused group ("fused", [(Co, KH, KW)...], Ci): members as
# ConvLayer.finalize_descs lays them out over one slab
FIN_SHAPES = [
    ("1x1 Ci128", 1, 16, 128, 128, 1, 1),
    ("1x1 Ci256", 1, 8, 256, 256, 1, 1),
    ("1x1 Ci264", 1, 16, 264, 264, 1, 1),
    ("3x3 Ci24", 1, 16, 24, 24, 3, 3),
    ("3x3 Ci32", 1, 24, 32, 32, 3, 3),
    ("7x7 Ci8", 1, 8, 8, 8, 7, 7),
    ("3x3 Ci3 Cs8", 1, 16, 3, 8, 3, 3),
    ("virtual stem", 1, 16, 7, 8, 1, 7),
    ("1x7", 1, 8, 16, 16, 1, 7),
    ("5x5", 1, 16, 8, 8, 5, 5),
    ("3x3 Ci8", 1, 8, 8, 8, 3, 3),
    ("G2 3x3", 2, 8, 16, 16, 3, 3),
    ("fused 3x3+1x1", [(16, 3, 3), (8, 1, 1)], 16),
    ("fused 1x1+1x1", [(8, 1, 1), (16, 1, 1)], 24),
]
FIN_GGS_EXTRA = 40  # the groups of "G2 3x3" lie this many elements further apart than one weight


def fin_descs(rot):
    """The finalize problems of part B: a list of dicts, one per SLAB, with its split count (FIN_SPLITS rotated by
    ``rot`` over the shapes) and its ``members`` [(Co, KH, KW, n0, t0)] (row and tap offset in the slab)."""
    out = []
    for i, s in enumerate(FIN_SHAPES):
        splits = FIN_SPLITS[(i + rot) % len(FIN_SPLITS)]
        if isinstance(s[1], list):
            (Co0, KH, KW), Ci = s[1][0], s[2]
            members, n0 = [], 0
            for Co, kh, kw in s[1]:
                members.append((Co, kh, kw, n0, ((KH - kh) // 2) * KW + (KW - kw) // 2))
                n0 += Co
            out.append({"name": s[0], "G": 1, "Co": n0, "Ci": Ci, "Cs": Ci, "KH": KH, "KW": KW, "splits": splits,
                        "members": members})
        else:
            _, G, Co, Ci, Cs, KH, KW = s
            out.append({"name": s[0], "G": G, "Co": Co, "Ci": Ci, "Cs": Cs, "KH": KH, "KW": KW, "splits": splits,
                        "members": [(Co, KH, KW, 0, 0)]})
    for d in out:
        d["Npad"], d["Kpad"] = pad_to(d["Co"], 16), pad_to(d["KH"] * d["KW"] * d["Cs"], 64)
    return out


def fin_slab(d, seed):
    """The slab [G, splits, Npad, Kpad] of one finalize problem: integers |v| <= 64 where some member's gradient
    reads, NaN everywhere else (rows >= Co, columns >= taps * Cs, channels >= Ci, the other taps of a centre-tap
    member's rows)."""
    g = gen(2000 + seed)
    slab = torch.full((d["G"], d["splits"], d["Npad"], d["Kpad"]), NAN)
    for Co, kh, kw, n0, t0 in d["members"]:
        for t in range(kh * kw):
            k0 = (t0 + t) * d["Cs"]
            slab[:, :, n0:n0 + Co, k0:k0 + d["Ci"]] = ints(g, (d["G"], d["splits"], Co, d["Ci"]), 64, 0.1)
    return slab


def fin_ref(slab, d, member, scale, skip_split=None):
    """fp64 gradient [G, Co, Ci, kh, kw] of one member: the sum over splits times ``scale``."""
    Co, kh, kw, n0, t0 = member
    s = slab.double()
    if skip_split is not None:
        s = s[:, [i for i in range(s.shape[1]) if i != skip_split]]
    k0 = t0 * d["Cs"]
    v = s.sum(1)[:, n0:n0 + Co, k0:k0 + kh * kw * d["Cs"]].reshape(d["G"], Co, kh * kw, d["Cs"])[..., :d["Ci"]]
    return (v * scale).permute(0, 1, 3, 2).reshape(d["G"], Co, d["Ci"], kh, kw)


# ---------------------------------------------------------------------------------------------------
# C. Adam + pack
def f32(x):
    """A hyperparameter as the kernel holds it: rounded to fp32, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def adam_ref(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, grad_scale=1.0, decoupled=False):
    """One fp64 Adam step with coupled L2 from fp32 inputs and fp32-rounded hyperparameters (``lr`` is an fp32 device
    scalar already).  Returns p, m, v and the magnitudes of the two addends of m and of v.  ``decoupled``: AdamW's
    decay instead (the sensitivity tests' wrong reference)."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2, eps, wd, gs, lr = (f32(x) for x in (b1, b2, eps, wd, grad_scale, lr))
    gj = g * gs + (0.0 if decoupled else wd * p)
    a1, a2 = b1 * m, (1.0 - b1) * gj
    q1, q2 = b2 * v, (1.0 - b2) * gj * gj
    mn, vn = a1 + a2, q1 + q2
    pn = (p * (1.0 - lr * wd) if decoupled else p) + adam_update(mn, vn, t, lr, b1, b2, eps)
    return {"p": pn, "m": mn, "v": vn, "m_mag": a1.abs() + a2.abs(), "v_mag": q1.abs() + q2.abs()}


def adam_update(m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """The fp64 update p_new - p_old from the moments AFTER the step (fp32-rounded hyperparameters)."""
    b1, b2, eps, lr = (f32(x) for x in (b1, b2, eps, lr))
    return -(lr / (1.0 - b1 ** t)) * m.double() / (v.double().sqrt() / math.sqrt(1.0 - b2 ** t) + eps)


def adam_tau(t, b1=0.9, b2=0.999):
    """Relative bound of the fp32 update: the cancellation in 1 - powf(b, t) for both moments plus 8 roundings."""
    b1, b2 = f32(b1), f32(b2)
    return 4 * 2.0 ** -24 * (1.0 / (1.0 - b1 ** t) + 1.0 / (1.0 - b2 ** t)) + 8 * 2.0 ** -24


def adam_state(n, seed):
    """fp32 p, g, m, v of ``n`` elements: |p| in [0.5, 1.5], |g| in [0.25e-2, 4e-2], |m| ~ 1e-2 away from zero,
    v in [0.25e-4, 1.25e-4] -- every term of the step moves the result, and |g * grad_scale| >= 16 |wd * p| down to
    grad_scale = 1/8 at wd = 1e-5, so that neither sum of the step cancels."""
    g_ = gen(3000 + seed)

    def sign():
        return torch.randint(0, 2, (n,), generator=g_).float() * 2 - 1
    p = sign() * (0.5 + torch.rand(n, generator=g_))
    g = sign() * 0.25e-2 * 16 ** torch.rand(n, generator=g_)
    m = sign() * 1e-2 * (0.25 + torch.rand(n, generator=g_))
    v = 1e-4 * (0.25 + torch.rand(n, generator=g_))
    return p, g, m, v


# (name, Co, Ci, KH, KW, Cs) conv weights of part C; fused groups as in FIN_SHAPES
OPT_CONVS = [
    ("3x3 8x8", 8, 8, 3, 3, 8),
    ("3x3 24x40", 24, 40, 3, 3, 40),
    ("3x3 Ci3 Cs8", 16, 3, 3, 3, 8),
    ("1x1 Ci264", 16, 264, 1, 1, 264),
    ("7x7", 8, 8, 7, 7, 8),
    ("5x5", 16, 16, 5, 5, 16),
    ("1x7 Ci64", 16, 64, 1, 7, 64),
    ("virtual stem", 16, 7, 1, 7, 8),
    ("fused 3x3+1x1", [(16, 3, 3), (8, 1, 1)], 16),
    ("fused 1x1+1x1", [(8, 1, 1), (16, 1, 1)], 24),
]
OPT_PLAIN = [4, 1020, 1024, 1028, 8, 4, 12, 4, 4, 4, 8, 4, 1500]  # plain ranges before each weight, after the last


def opt_layout():
    """The flat buffer of part C: plain ranges of OPT_PLAIN between the members' weights.  Returns (numel, images):
    ``images`` one dict per conv / fused group with Co, Ci, Cs, KH, KW, Npad, Kpad (forward image), Npad_d, Kpad_d
    (data-gradient image) and ``members`` [(Co, kh, kw, n0, t0, flat offset)]."""
    pos, images, gaps = 0, [], iter(OPT_PLAIN)
    for s in OPT_CONVS:
        if isinstance(s[1], list):
            (_, KH, KW), Ci, Cs = s[1][0], s[2], s[2]
            mem = [(Co, kh, kw, ((KH - kh) // 2) * KW + (KW - kw) // 2) for Co, kh, kw in s[1]]
        else:
            _, Co, Ci, KH, KW, Cs = s
            mem = [(Co, KH, KW, 0)]
        members, n0 = [], 0
        for Co, kh, kw, t0 in mem:
            pos += next(gaps)
            members.append((Co, kh, kw, n0, t0, pos))
            pos += Co * Ci * kh * kw
            n0 += Co
        taps = KH * KW
        images.append({"name": s[0], "Co": n0, "Ci": Ci, "Cs": Cs, "KH": KH, "KW": KW, "members": members,
                       "Npad": pad_to(n0, 16), "Kpad": pad_to(taps * Cs, 32), "Npad_d": pad_to(Cs, 16),
                       "Kpad_d": pad_to(taps * n0, 32)})
    pos += next(gaps)
    assert pos % 4 == 0 and pos % 1024, pos
    return pos, images


def pack_fwd_ref(w, Cs):
    """bf16 forward image [Co, taps * Cs] of w [Co, Ci, kh, kw] (column = tap * Cs + ci; channels >= Ci zero)."""
    Co, Ci, kh, kw = w.shape
    t = torch.zeros(Co, kh * kw, Cs, dtype=w.dtype, device=w.device)
    t[..., :Ci] = w.reshape(Co, Ci, kh * kw).permute(0, 2, 1)
    return t.reshape(Co, kh * kw * Cs).bfloat16()


def image_refs(im, p, fill_f, fill_d):
    """The two images of one conv / fused group from the flat masters ``p``: every member embedded at its row, tap
    and column offset into copies of ``fill_f`` [Npad, Kpad] / ``fill_d`` [Npad_d, Kpad_d] (what the buffers held)."""
    wf, wd = fill_f.clone(), fill_d.clone()
    for Co, kh, kw, n0, t0, off in im["members"]:
        w = p[off:off + Co * im["Ci"] * kh * kw].view(Co, im["Ci"], kh, kw)
        k0 = t0 * im["Cs"]
        wf[n0:n0 + Co, k0:k0 + kh * kw * im["Cs"]] = pack_fwd_ref(w, im["Cs"])
        for t in range(kh * kw):
            c0 = (t0 + t) * im["Co"] + n0
            wd[:im["Ci"], c0:c0 + Co] = w.reshape(Co, im["Ci"], kh * kw)[:, :, t].t().bfloat16()
    return wf, wd


# ---------------------------------------------------------------------------------------------------
# D. packed-tap stem
# (KH, KW, stride, padding, H, W)
STEMS = [(7, 7, 3, 2, 20, 31), (3, 3, 2, 0, 17, 30)]


def pack_taps_ref(X, idx, taps, off):
    """bf16 [B, H, W, 8]: channel j of pixel (h, w) = bf16(X[idx, 0, h - off + j, w]), zero outside the image and for
    j >= taps (X [N, 1, H, W] fp32)."""
    N, _, H, W = X.shape
    out = torch.zeros(len(idx), H, W, 8)
    for j in range(taps):
        lo, hi = max(0, off - j), min(H, H + off - j)   # rows h with 0 <= h - off + j < H
        out[:, lo:hi, :, j] = X[idx, 0, lo - off + j:hi - off + j, :]
    return out.bfloat16()


# ---------------------------------------------------------------------------------------------------
class Checker:
    """Collects every violated bound, naming the worst offending element, and the worst observed value of each kind
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
        """Bit-for-bit after a cast to fp64 (a NaN on either side is a mismatch)."""
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
        """Two bf16 tensors bit for bit."""
        return self.exact(what, got.contiguous().view(torch.int16), ref.to(got.device).contiguous().view(torch.int16))

    def bounded(self, kind, what, got, ref, bound):
        """|got - ref| <= bound per element (fp64); records max err / bound."""
        ref, bound = ref.to(got.device), bound.to(got.device)
        err = (got.double() - ref).abs()
        ratio = err / bound.clamp_min(1e-300)
        ok = err <= bound
        self._note(kind + " err / bound", float(ratio[torch.isfinite(ratio)].max()) if bool(torch.isfinite(ratio).any()) else 0.0)
        if not bool(ok.all()):
            at = self._where(~ok)
            self.bad.append((what, kind, f"{int((~ok).sum())} elements out of bound, first at {at}: got "
                             f"{got[at].item()!r} ref {ref[at].item()!r} bound {bound[at].item():.3e}"))
            return False
        return True

    def wgrad_real(self, what, got, ref, T, n):
        """A real-valued weight gradient: |got - ref| <= 2 n 2^-24 T, T the gradient of (|x|, |dy|)."""
        return self.bounded("wgrad", what, got, ref, 2.0 * n * 2.0 ** -24 * T)

    def adam(self, what, got, old, t, lr, **hp):
        """One Adam step: ``got`` / ``old`` dicts of fp32 p, g (old only), m, v.  m and v against the fp64 step within
        4 * 2^-24 of their addends' magnitudes; the update p_new - p_old against the fp64 formula on the kernel's own
        stored m, v within adam_tau(t) |update| + 2^-24 |p|."""
        hp2 = {k: v for k, v in hp.items() if k in ("b1", "b2", "eps")}
        r = adam_ref(old["p"], old["g"], old["m"], old["v"], t, lr, **hp)
        ok = self.bounded("adam m", what, got["m"], r["m"], 4 * 2.0 ** -24 * r["m_mag"])
        ok &= self.bounded("adam v", what, got["v"], r["v"], 4 * 2.0 ** -24 * r["v_mag"])
        upd = adam_update(got["m"], got["v"], t, lr, **hp2)
        bound = adam_tau(t, hp.get("b1", 0.9), hp.get("b2", 0.999)) * upd.abs() + 2.0 ** -24 * old["p"].double().abs()
        ok &= self.bounded("adam update", what, got["p"].double() - old["p"].double(), upd, bound)
        return ok

    def true(self, what, cond):
        if not cond:
            self.bad.append((what, "condition"))
        return bool(cond)

    def done(self):
        print("worst observed", {k: f"{v:.2e}" for k, v in self.worst.items()}, "exact comparisons", self.count)
        assert not self.bad, self.bad[:20]
