"""Plain fp64 reference and input builders of the data gradient of a convolution (tests/test_dgrad_gpu.py; checked on
the CPU by tests/test_dgrad_ref.py).  CPU torch only; nothing here imports the extension.

The reference is a scatter, tap by tap: every dy[b, oh, ow, :] @ w[:, :, kh, kw] is added at input pixel
(oh sh - ph + kh, ow sw - pw + kw) when that lies inside the map -- no conv_transpose2d, no phases, no flipped
weights, so it shares no index arithmetic with the kernels' gather and sub-pixel forms.

With integer-valued inputs (dy in [-4, 4], w in [-2, 2] -- [-1, 1] for 5x5 --, sources in [-4, 4]; all exact in bf16)
every product and every partial sum of an element, in any order and under any split of K, is an integer below
T = dgrad(|dy|, |w|) + sum|sources| < 2^24: the fp32 accumulator is exact and the stored dx must equal
bf16_rne(reference) bit for bit.  Real-valued inputs are held to |err| <= 2^-8 |ref| + K 2^-24 T per element (one
bf16 ulp plus the worst case of an fp32 accumulation of K = KH KW Co + sources addends).

The flat buffers, their views, the guard rows and the Checker are those of tests/fwd_ref.py, addressed through the
two layout records of a case (``DCase.dyl``: dy as a conv input, ``DCase.dxl``: dx as a conv output).
"""
from dataclasses import dataclass, field
from types import SimpleNamespace

import torch

import fwd_ref as R
from wpath_ref import NAN, SENT, gen, ints  # noqa: F401  (re-exported for the tests)


@dataclass
class DCase:
    """One data gradient as the kernels address it: the conv (B, H, W, Ci) -> (B, Ho, Wo, Co), its input stored
    with Cs >= Ci channels (``cin_stored``; dx channels Ci..Cs carry no weight).  dy is the slice [doff, doff + Co)
    of a buffer of pitch ldd, dx the slice [ooff, ooff + Cs) of a buffer of pitch ldo; G groups whose dy buffers lie
    ``dgap`` and whose dx buffers ``ogap`` elements further apart than one group's buffer; ``nsrc`` added gradient
    sources of dx's shape."""
    name: str
    B: int
    H: int
    W: int
    Ci: int
    Co: int
    Cs: int = 0
    KH: int = 3
    KW: int = 3
    sh: int = 1
    sw: int = 1
    ph: int = 1
    pw: int = 1
    G: int = 1
    nsrc: int = 0
    ldd: int = 0
    doff: int = 0
    dgap: int = 0
    ldo: int = 0
    ooff: int = 0
    ogap: int = 0
    real: bool = False       # randn data rounded to bf16 instead of integers
    wlim: int = 2            # integer weights in [-wlim, wlim]
    seed: int = 0
    Ho: int = field(init=False)
    Wo: int = field(init=False)

    def __post_init__(self):
        self.Cs = self.Cs or self.Ci
        self.ldd = self.ldd or self.Co
        self.ldo = self.ldo or self.Cs
        self.Ho = (self.H + 2 * self.ph - self.KH) // self.sh + 1
        self.Wo = (self.W + 2 * self.pw - self.KW) // self.sw + 1

    @property
    def M(self):
        """dx pixels of one group."""
        return self.B * self.H * self.W

    @property
    def K(self):
        """Addends of one dx element at most."""
        return self.KH * self.KW * self.Co + self.nsrc

    @property
    def dyl(self):
        """dy as fwd_ref addresses a conv input."""
        return SimpleNamespace(G=self.G, B=self.B, H=self.Ho, W=self.Wo, C0=self.Co, ld0=self.ldd, off0=self.doff,
                               gap=self.dgap)

    @property
    def dxl(self):
        """dx as fwd_ref addresses a conv output."""
        return SimpleNamespace(G=self.G, B=self.B, Ho=self.H, Wo=self.W, Co=self.Cs, ldo=self.ldo, ooff=self.ooff,
                               ogap=self.ogap, M=self.M)


def dy_view(buf, c: DCase):
    """The [G, B, Ho, Wo, Co] slice the dgrad reads of the flat dy buffer [G, pixels * ldd + dgap] (any device)."""
    return R.in_view(buf, c.dyl)


def dx_buf(c: DCase):
    """The flat bf16 dx buffer, SENT everywhere (guard rows, G groups of pixels * ldo + ogap, guard rows)."""
    return R.out_buf(c.dxl)


def dx_view(flat, c: DCase):
    """The [G, B, H, W, Cs] slice of :func:`dx_buf` (any device) the dgrad writes."""
    return R.out_view(flat, c.dxl)


def dx_foreign(flat, c: DCase):
    """Every element of the flat dx buffer outside the addressed slice (a 1-D copy): must still be SENT."""
    return R.out_foreign(flat, c.dxl)


def dgrad_inputs(c: DCase) -> dict:
    """``dybuf``: the bf16 buffer as the kernel reads it (NaN outside the slice); ``w`` fp32 [G, Co, Ci, KH, KW]
    holding bf16-exact values; ``srcs``: ``nsrc`` bf16 sources [G, B, H, W, Cs]; ``dy`` [G, B, Ho, Wo, Co] in
    fp64."""
    g = gen(11000 + c.seed)
    ds, ws, ss = (c.G, c.B, c.Ho, c.Wo, c.Co), (c.G, c.Co, c.Ci, c.KH, c.KW), (c.G, c.B, c.H, c.W, c.Cs)
    if c.real:
        dy = torch.randn(ds, generator=g).bfloat16().float()
        w = (torch.randn(ws, generator=g) / (c.KH * c.KW * c.Co) ** 0.5).bfloat16().float()
        srcs = [torch.randn(ss, generator=g).bfloat16() for _ in range(c.nsrc)]
    else:
        dy = ints(g, ds, 4)
        w = ints(g, ws, c.wlim, 0.375 if c.wlim > 1 else 0.25)
        srcs = [ints(g, ss, 4).bfloat16() for _ in range(c.nsrc)]
    return {"dybuf": R.in_buf(dy, c.dyl), "w": w, "srcs": srcs, "dy": dy.double()}


def scatter(dy, w, c: DCase, pad=None, drop=None):
    """fp64 data gradient of one group, tap by tap: dy [B, Ho, Wo, Co], w [Co, Ci, KH, KW] -> [B, H, W, Cs] (channels
    Ci..Cs zero).  ``pad`` = (ph, pw) to scatter with instead of the case's; ``drop`` = (kh, kw, ih, px): that tap
    leaves out row ``ih`` of dx at the columns of parity class ``px`` (mod sw) -- both only for the sensitivity
    tests' wrong references."""
    dy, w = dy.double(), w.double()
    ph, pw = (c.ph, c.pw) if pad is None else pad
    Ho, Wo = dy.shape[1:3]
    dx = torch.zeros(c.B, c.H, c.W, c.Cs, dtype=torch.float64)
    for kh in range(c.KH):
        for kw in range(c.KW):
            t = dy @ w[:, :, kh, kw]                                   # [B, Ho, Wo, Ci]
            for oh in range(Ho):
                ih = oh * c.sh - ph + kh
                if not 0 <= ih < c.H:
                    continue
                ows = [ow for ow in range(Wo) if 0 <= ow * c.sw - pw + kw < c.W]
                if drop is not None and drop[:3] == (kh, kw, ih):
                    ows = [ow for ow in ows if (ow * c.sw - pw + kw) % c.sw != drop[3]]
                if ows:
                    iws = [ow * c.sw - pw + kw for ow in ows]
                    dx[:, ih, iws, :c.Ci] += t[:, oh, ows]
    return dx


def dgrad(c: DCase, inp: dict) -> dict:
    """``dx`` [G, B, H, W, Cs]: the exact fp64 gradient plus the sources; ``dxbf``: its bf16 round-to-nearest-even
    image; ``T`` = dgrad(|dy|, |w|) + sum|sources|."""
    dx = torch.stack([scatter(inp["dy"][z], inp["w"][z], c) for z in range(c.G)])
    T = torch.stack([scatter(inp["dy"][z].abs(), inp["w"][z].abs(), c) for z in range(c.G)])
    for s in inp["srcs"]:
        dx = dx + s.double()
        T = T + s.double().abs()
    return {"dx": dx, "dxbf": R.bf16_rne(dx).float().bfloat16(), "T": T}


def randn_bound(c: DCase, ref: dict):
    """Per-element bound of a real-valued case: 2^-8 |ref| + K 2^-24 T."""
    return 2.0 ** -8 * ref["dx"].abs() + c.K * 2.0 ** -24 * ref["T"]


class Checker(R.Checker):
    """fwd_ref.Checker plus the composite checks of one dgrad launch (run against perturbed references on the
    CPU by tests/test_dgrad_ref.py)."""

    def dgrad_exact(self, what, c, flat, ref):
        """An integer launch: dx == bf16_rne(ref) bit for bit, finite (no poisoned column or gap read), every
        sentinel of the flat buffer ``flat`` outside the slice intact."""
        dx = dx_view(flat, c)
        ok = self.true(what + " finite", bool(torch.isfinite(dx.float()).all()))
        ok &= self.bits(what + " dx", dx.contiguous(), ref["dxbf"])
        ok &= self.sentinels(what + " dx sentinels", dx_foreign(flat, c))
        return ok

    def dgrad_bounded(self, what, c, flat, ref):
        """A real-valued launch: :func:`randn_bound` on every element, the sentinels intact."""
        ok = self.bounded("dx", what, dx_view(flat, c), ref["dx"], ref["bound"])
        ok &= self.sentinels(what + " dx sentinels", dx_foreign(flat, c))
        return ok


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_dgrad_gpu.py: the smallest shapes at which each mechanism can still go wrong
BASE = (2, 17, 42)


def _c(name, shape, Ci, Co, **kw):
    return DCase(name, *shape, Ci, Co, **kw)


_V = dict(ph=0, pw=0)
_S2 = dict(sh=2, sw=2)
ICASES = [
    _c("3x3 p1", BASE, 32, 48, nsrc=2, seed=1),
    _c("3x3 p1 Cs24", BASE, 24, 48, seed=2),                      # N below / above a tile's BN, no multiple of it
    _c("3x3 p1 Cs80", BASE, 80, 48, seed=3),
    _c("3x3 p1 Co40", BASE, 32, 40, seed=4),                      # K = 360: no multiple of 32
    _c("3x3 p1 Co8", BASE, 32, 8, nsrc=1, seed=5),                # K = 72
    _c("3x3 p0", (2, 10, 28), 32, 32, **_V, seed=6),              # the patch kernels' halo-2 form
    _c("3x3 s2 odd", (2, 17, 41), 32, 48, **_S2, seed=7),         # phases of different Hq, Wq
    _c("3x3 s2 even", (2, 8, 12), 32, 48, **_S2, seed=8),
    _c("3x3 s2 one row", (3, 1, 6), 32, 48, **_S2, seed=9),       # fewer phases than the stride
    _c("3x3 s2 p0 leftover", (2, 8, 12), 32, 48, **_S2, **_V, seed=10),      # row 7, column 11 under no window
    _c("3x3 s2 p0 leftover src", (2, 8, 12), 32, 48, **_S2, **_V, nsrc=1, seed=11),
    _c("3x3 s2 p0 fit", (2, 9, 27), 32, 48, **_S2, **_V, seed=12),
    _c("1x1 s2", BASE, 32, 16, KH=1, KW=1, **_S2, **_V, seed=13),            # three empty phases, K one chunk
    _c("1x1 s2 src", BASE, 32, 16, KH=1, KW=1, **_S2, **_V, nsrc=1, seed=14),
    _c("1x1 Co256", (2, 5, 11), 64, 256, KH=1, KW=1, **_V, seed=15),
    _c("5x5 p2", (2, 10, 28), 32, 48, KH=5, KW=5, ph=2, pw=2, wlim=1, seed=16),
    _c("1x7", (2, 4, 13), 128, 192, KH=1, KW=7, ph=0, pw=3, seed=17),
    _c("7x1", (2, 4, 13), 128, 192, KH=7, KW=1, ph=3, pw=0, seed=18),
    _c("B1 1x6", (1, 1, 6), 32, 32, nsrc=1, seed=19),             # M below any tile
    _c("cin8 Ci1", (2, 9, 21), 1, 32, Cs=8, seed=20),
    _c("cin8 Ci3", (2, 9, 21), 3, 32, Cs=8, nsrc=1, seed=21),
    _c("pitched dy", BASE, 32, 32, ldd=96, doff=16, seed=22),
    _c("dx slice", BASE, 32, 32, ldo=64, ooff=8, nsrc=1, seed=23),
    _c("G3 gaps", (2, 9, 21), 32, 32, G=3, ldd=40, doff=8, dgap=16, ogap=8, nsrc=1, seed=24),
]
# strides no model uses: a config refuses them at prepare time or is exact
UCASES = [
    _c("3x3 s(2,1)", (2, 9, 21), 32, 32, sh=2, sw=1, seed=25),
    _c("3x3 s3", (2, 10, 22), 32, 32, sh=3, sw=3, seed=26),
]
RCASES = [
    _c("real 3x3 s2", (2, 17, 41), 32, 48, **_S2, nsrc=1, real=True, seed=31),
    _c("real 1x7", (2, 4, 13), 128, 192, KH=1, KW=7, ph=0, pw=3, real=True, seed=32),
]
DCASES = {c.name: c for c in ICASES + UCASES + RCASES}
XCD_CASES = ("3x3 s2 odd", "3x3 p0")
