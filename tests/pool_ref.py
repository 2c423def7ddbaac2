"""Plain fp64 references and input builders of the Inception pools (tests/test_pools_gpu.py; checked on the CPU by
tests/test_pool_ref.py against torch's own pools and their autograd): max 3x3 / stride 2 / no padding with its window
argmax, average 3x3 / stride 1 / padding 1 always divided by 9, and the backward of both from up to 6 gradient
sources.  Explicit loops over the nine window positions on NHWC tensors; plain torch ops, so the functions run on any
device; nothing here imports the extension.

Rules of the max pool (torch's, as tests/test_pool_ref.py shows): the first maximum of a window in row-major order
wins; a NaN wins over everything and the LAST NaN of a window gives the position; a window of -inf gives -inf at
position 0.

Integer-valued inputs (|v| <= 4) make every result exact: a maximum is one of its inputs; a gradient is a sum of at
most 6 sources x 9 windows = 54 integers, |S| <= 216 < 2^24, exact in fp32 in any order; a max-pool gradient
(at most 4 windows x 6 sources, |S| <= 96 < 256) is exact in bf16 as well, and S / 9 is rounded once.
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import torch

from fwd_ref import bf16_rne, one_ulp, ulp_bf16
from wpath_ref import NAN, SENT, gen, ints

GRID_ITEMS = 4096 * 256   # work items one trip of the kernels' grid covers
EXCLUDED_CAP = 0.005      # share of elements that may lie too near a bf16 rounding boundary to demand one neighbour


# ---------------------------------------------------------------------------------------------------
# definitions (x, g: [B, H, W, C] / [B, Ho, Wo, C], fp64)
def max_out_hw(H, W):
    return (H - 3) // 2 + 1, (W - 3) // 2 + 1


def _win(t, kh, kw, Ho, Wo):
    """The elements at window position (kh, kw) of every stride-2 window: a [B, Ho, Wo, C] view of t [B, H, W, C]."""
    return t[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]


def max_fwd(x):
    """(y, am): the window maximum and its position 0..8 (row-major) under the rules above."""
    B, H, W, C = x.shape
    Ho, Wo = max_out_hw(H, W)
    y = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64, device=x.device)
    am = torch.zeros((B, Ho, Wo, C), dtype=torch.int64, device=x.device)
    for t in range(9):
        v = _win(x.double(), t // 3, t % 3, Ho, Wo)
        take = (v > y) | torch.isnan(v)
        y = torch.where(take, v, y)
        am = torch.where(take, torch.full_like(am, t), am)
    return y, am


def max_bwd(g, am, H, W):
    """dx [B, H, W, C]: every window's gradient goes to its argmax; pixels covered by no window stay exactly 0."""
    B, Ho, Wo, C = g.shape
    dx = torch.zeros((B, H, W, C), dtype=torch.float64, device=g.device)
    for t in range(9):
        _win(dx, t // 3, t % 3, Ho, Wo).add_(torch.where(am == t, g.double(), torch.zeros_like(g, dtype=torch.float64)))
    return dx


def _sum9(t):
    """Sum of the 3x3 neighbourhood (zero outside the map) of every pixel of t [B, H, W, C]."""
    B, H, W, C = t.shape
    p = torch.zeros((B, H + 2, W + 2, C), dtype=torch.float64, device=t.device)
    p[:, 1:H + 1, 1:W + 1] = t
    s = torch.zeros((B, H, W, C), dtype=torch.float64, device=t.device)
    for k in range(9):
        s += p[:, k // 3:k // 3 + H, k % 3:k % 3 + W]
    return s


def avg_fwd(x):
    return _sum9(x.double()) / 9.0


def avg_bwd(g):
    """The output windows covering input pixel (h, w) are the outputs (h - 1 .. h + 1, w - 1 .. w + 1): the same sum."""
    return _sum9(g.double()) / 9.0


# ---------------------------------------------------------------------------------------------------
# layout
def sliced(vals, ld, off, fill):
    """``vals`` [..., C] (fp32 / fp64) as the channel slice [off, off + C) of a [M][ld] fp32 buffer (M = the product of
    the leading dimensions) whose every other element is ``fill``: NAN where a launch may not read, SENT where it may
    not write."""
    C = vals.shape[-1]
    M = vals.numel() // C
    buf = torch.full((M, ld), fill, dtype=torch.float32, device=vals.device)
    buf[:, off:off + C] = vals.reshape(M, C).float()
    return buf


def owned(buf2d, off, C):
    """(the addressed slice, a 1-D copy of everything else) of a [M][ld] buffer."""
    mask = torch.ones(buf2d.shape, dtype=torch.bool, device=buf2d.device)
    mask[:, off:off + C] = False
    return buf2d[:, off:off + C], buf2d[mask]


# ---------------------------------------------------------------------------------------------------
# rounding
def boundary_distance(ref):
    """Distance (fp64) of ``ref`` from the nearest bf16 rounding boundary, i.e. the nearer of the two midpoints between
    bf16_rne(ref) and its neighbours (the lower neighbour of a power of two is half a step away)."""
    a = ref.double().abs()
    r = bf16_rne(a)
    u = ulp_bf16(r)
    m, _ = torch.frexp(r)
    down = torch.where(m == 0.5, u / 4, u / 2)
    return torch.minimum((r + u / 2 - a).abs(), (a - (r - down)).abs())


def determinate(ref, sumabs, k):
    """Where the stored bf16 must equal bf16_rne(ref): ref farther than k 2^-23 sum|terms| from a rounding boundary
    (k fp32 additions), or no rounding at all (every term zero: pixels no window covers, all-zero sources)."""
    return (boundary_distance(ref) > k * 2.0 ** -23 * sumabs) | (sumabs == 0)


# ---------------------------------------------------------------------------------------------------
# cases
@dataclass
class PCase:
    """One pool problem as the kernels address it: x, y and dx channel slices [off, off + C) of buffers of pitch ld,
    and ``srcs`` gradient sources (ld, off) of the output's shape, source ``zero_src`` all zeros."""
    kind: str                 # "max" / "avg"
    B: int
    H: int
    W: int
    C: int
    nsrc: int
    real: bool = False        # bf16-rounded randn instead of integers
    special: bool = False     # max pool: NaNs, a -inf window, a constant patch planted in x
    seed: int = 0
    ld: int = field(init=False)
    off: int = field(init=False)
    srcs: List[Tuple[int, int]] = field(init=False)
    zero_src: int = field(init=False)

    def __post_init__(self):
        # C = 8: one contiguous channel group; 24: slice 8.. of 40; 72: slice 16.. of 96 (sources too)
        self.ld, self.off = {8: (8, 0), 24: (40, 8), 72: (96, 16)}[self.C]
        if self.C == 72:
            self.srcs = [(96, 16)] * self.nsrc
        else:  # every source its own pitch and channel offset
            self.srcs = [(self.C + 8 * (i % 3 + 1), 8 * ((i + 1) % (i % 3 + 2))) for i in range(self.nsrc)]
        self.zero_src = self.nsrc - 1 if self.nsrc > 1 else -1
        assert all(o + self.C <= ld for ld, o in self.srcs)

    @property
    def is_max(self):
        return self.kind == "max"

    @property
    def out_hw(self):
        return max_out_hw(self.H, self.W) if self.is_max else (self.H, self.W)

    @property
    def name(self):
        return (f"{self.kind} {self.B}x{self.H}x{self.W}x{self.C} {self.nsrc} src "
                f"{'real' if self.real else 'int'}{' special' if self.special else ''}")


# one launch per kernel instantiation with more work items than one trip of the grid (forward: B Ho Wo C / 8,
# backward: B H W C / 8): name -> (is_max, backward, B, H, W, C)
GRID_CASES = {"max forward": (1, 0, 8, 97, 97, 512), "average forward": (0, 0, 2, 97, 97, 512),
              "average backward": (0, 1, 2, 97, 97, 512), "max backward, stored argmax": (1, 1, 2, 97, 97, 512),
              "max backward, windows re-read": (1, 1, 2, 97, 97, 512)}

MAX_MAPS = [(3, 3), (4, 7), (5, 6), (8, 9), (7, 3)]
AVG_MAPS = [(1, 9), (9, 1), (2, 2), (3, 5), (6, 7)]
SPECIAL_MAP = (8, 9)


def cases(kind, hw):
    """Every (B, C, sources, integer / real) combination of one map; the specials ride on the 8 x 9 max map."""
    out = []
    for B in (1, 3):
        for C in (8, 24, 72):
            for nsrc in (1, 2, 6):
                for real in (False, True):
                    out.append(PCase(kind, B, hw[0], hw[1], C, nsrc, real=real,
                                     seed=hw[0] * 100 + hw[1] * 10 + B + C + nsrc))
    if kind == "max" and hw == SPECIAL_MAP:
        out += [PCase(kind, B, hw[0], hw[1], 24, n, special=True, seed=900 + B + n) for B in (1, 3) for n in (1, 6)]
    return out


def uncovered(H, W):
    """[H, W] bool: the pixels no max-pool window covers (the last row / column of an even map)."""
    Ho, Wo = max_out_hw(H, W)
    m = torch.ones(H, W, dtype=torch.bool)
    m[:2 * Ho + 1, :2 * Wo + 1] = False
    return m


def inputs(c: PCase) -> dict:
    """``x`` [B, H, W, C] and the gradient sources ``g`` [n][B, Ho, Wo, C] in fp32 (all values exact in bf16).  Max
    pool: the pixels no window covers are NaN.  Specials (8 x 9 map, channels 1-4 of every image): a NaN at (2, 2),
    which four windows cover; two NaNs, (0, 0) and (1, 1), in window (0, 0) alone; window (1, 2) all -inf; a constant
    6 x 6 patch."""
    g = gen(5000 + c.seed)
    Ho, Wo = c.out_hw
    if c.real:
        x = torch.randn(c.B, c.H, c.W, c.C, generator=g).bfloat16().float()
        gs = [torch.randn(c.B, Ho, Wo, c.C, generator=g).bfloat16().float() for _ in range(c.nsrc)]
    else:
        x = ints(g, (c.B, c.H, c.W, c.C))
        gs = [ints(g, (c.B, Ho, Wo, c.C)) for _ in range(c.nsrc)]
    if c.zero_src >= 0:
        gs[c.zero_src] = torch.zeros_like(gs[c.zero_src])
    if c.special:
        x[:, 2, 2, 1] = NAN
        x[:, 0, 0, 2] = NAN
        x[:, 1, 1, 2] = NAN
        x[:, 2:5, 4:7, 3] = float("-inf")
        x[:, :6, :6, 4] = 2.0
    if c.is_max:
        x[:, uncovered(c.H, c.W)] = NAN
    return {"x": x, "g": gs}


def _grain(t):
    """The power of two every bf16 value of ``t`` is a multiple of, element by element (inf for a zero)."""
    u = ulp_bf16(t.double())
    return torch.where(u == 0, torch.full_like(u, float("inf")), u)


def _min9(t):
    """Minimum over the 3x3 neighbourhood (inf outside the map)."""
    B, H, W, C = t.shape
    p = torch.full((B, H + 2, W + 2, C), float("inf"), dtype=torch.float64, device=t.device)
    p[:, 1:H + 1, 1:W + 1] = t
    s = torch.full((B, H, W, C), float("inf"), dtype=torch.float64, device=t.device)
    for k in range(9):
        s = torch.minimum(s, p[:, k // 3:k // 3 + H, k % 3:k % 3 + W])
    return s


def _max_bwd_min(q, am, H, W):
    """max_bwd with a minimum in place of the sum (inf where nothing is routed)."""
    B, Ho, Wo, C = q.shape
    out = torch.full((B, H, W, C), float("inf"), dtype=torch.float64, device=q.device)
    for t in range(9):
        v = _win(out, t // 3, t % 3, Ho, Wo)
        v.copy_(torch.minimum(v, torch.where(am == t, q, torch.full_like(q, float("inf")))))
    return out


def reference(c: PCase, inp: dict) -> dict:
    """fp64: ``y`` (and ``am`` for max), ``dx`` from the summed sources; per result r in (y, dx): ``r_sum`` the sum
    before the average's division (the result itself for max), ``r_abs`` the sum of the absolute terms of the result
    (the same operation on |x| / sum |g_i|), ``r_grain`` the smallest grain of its non-zero terms."""
    x = inp["x"].double()
    gs = torch.stack([t.double() for t in inp["g"]])
    gsum, gabs, ggrain = gs.sum(0), gs.abs().sum(0), _grain(gs).amin(0)
    if c.is_max:
        y, am = max_fwd(x)
        dx = max_bwd(gsum, am, c.H, c.W)
        return {"y": y, "am": am, "dx": dx, "dx_sum": dx, "dx_abs": max_bwd(gabs, am, c.H, c.W),
                "dx_grain": _max_bwd_min(ggrain, am, c.H, c.W)}
    return {"y": avg_fwd(x), "y_sum": _sum9(x), "y_abs": avg_fwd(x.abs()), "y_grain": _min9(_grain(x)),
            "dx": avg_bwd(gsum), "dx_sum": _sum9(gsum), "dx_abs": avg_bwd(gabs), "dx_grain": _min9(ggrain)}


def additions(c: PCase, backward: bool) -> int:
    """fp32 additions behind one stored element: 9 window positions (4 covering windows for the max-pool gradient) per
    source; a maximum is not rounded at all."""
    if not backward:
        return 0 if c.is_max else 9
    return (4 if c.is_max else 9) * c.nsrc


def sum_is_exact(total_abs, grain):
    """Where an fp32 sum of the terms is exact in ANY order: every term, hence every partial sum, is a multiple of
    ``grain``, and no partial sum exceeds ``total_abs`` < 2^24 grain."""
    return total_abs < 2.0 ** 24 * grain


def check_real(chk, c, r, got, ref):
    """A real-valued result ``got`` (the stored bf16 of result ``r`` = "y" / "dx" of case ``c``; any dtype) against the
    references ``ref``.  Everywhere: within one bf16 ulp of the fp64 value.  Where the value is farther than
    k 2^-23 sum|terms| from a rounding boundary (``determinate``): its nearest bf16.  Where it is not, but the fp32 sum
    is exact in any order (``sum_is_exact``: bf16 data often ties exactly, 1-3 % of these elements), the rounding of
    the exact arithmetic: bf16_rne(sum) for the max pool, bf16(fp32(sum x fp32(1/9))) for the average.  Returns the
    share of elements left with the one-ulp bound alone."""
    what = f"{c.name} {r}"
    v, total, k = ref[r], ref[r + "_abs"], additions(c, r == "dx")
    det = determinate(v, total, k)
    want = bf16_rne(v)
    if c.is_max:
        exact = sum_is_exact(total, ref[r + "_grain"])
    else:
        exact = sum_is_exact(9.0 * total, ref[r + "_grain"])
        ninth = torch.tensor(1.0 / 9.0, dtype=torch.float32).double().to(v.device)
        want = torch.where(exact, (ref[r + "_sum"] * ninth).float().bfloat16().double(), want)  # 24 x 24 bits: exact in fp64
    must = det | exact
    chk.bounded("ulp", what, got, v, one_ulp(v))
    chk.exact(what + " (nearest bf16)", got.double()[must], want[must])
    return 1.0 - float(must.double().mean())

