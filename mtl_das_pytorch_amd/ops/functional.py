"""Functional (tensor-in / tensor-out) entry points to the HIP kernels.

These are the stand-alone versions of what the engine launches from prebuilt programs; they are used by
the kernel numerics tests and are convenient for experimentation.  All activations are NHWC
(``[B, H, W, C]``) on the GPU; weights use the reference PyTorch layout ``[Co, Ci, KH, KW]`` (fp32).
Every function requires a CUDA (ROCm) tensor and the built extension -- there is no silent fallback.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .hip import lib, ptr, stream

# copies of csrc constants; tests/test_wgrad_configs.py compares every one with what the extension exports
NREP = 32


def _pad(x, m):
    return (x + m - 1) // m * m


def _grad(g: torch.Tensor) -> torch.Tensor:
    """An activation gradient as the kernels read it: contiguous bf16 (csrc/common.h GradSrcs)."""
    if not g.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    return g.to(torch.bfloat16).contiguous()


def _check(t: torch.Tensor, dtype=None):
    if not t.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")


def pack_weight_fwd(w: torch.Tensor, cin_stored: Optional[int] = None) -> torch.Tensor:
    Co, Ci, KH, KW = w.shape
    Cs = cin_stored or Ci
    t = torch.zeros(Co, KH, KW, Cs, device=w.device)
    t[..., :Ci] = w.permute(0, 2, 3, 1)
    K = KH * KW * Cs
    out = torch.zeros(_pad(Co, 16), _pad(K, 32), device=w.device, dtype=torch.bfloat16)
    out[:Co, :K] = t.reshape(Co, K).to(torch.bfloat16)
    return out


def pack_weight_dgrad(w: torch.Tensor, cin_stored: Optional[int] = None) -> torch.Tensor:
    Co, Ci, KH, KW = w.shape
    Cs = cin_stored or Ci
    K = KH * KW * Co
    out = torch.zeros(_pad(Cs, 16), _pad(K, 32), device=w.device, dtype=torch.bfloat16)
    out[:Ci, :K] = w.permute(1, 2, 3, 0).reshape(Ci, K).to(torch.bfloat16)
    return out


def _geom(x_shape, w_shape, stride, padding):
    B, H, W, _ = x_shape
    Co, Ci, KH, KW = w_shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    Ho = (H + 2 * ph - KH) // sh + 1
    Wo = (W + 2 * pw - KW) // sw + 1
    return B, H, W, Co, Ci, KH, KW, sh, sw, ph, pw, Ho, Wo


def _fwd_cfg(N, M):
    if N <= 16:
        return 0
    if N <= 32:
        return 1
    if N <= 64:
        return 2 if M >= 64 * 256 else 4
    return 3 if M >= 64 * 128 else 4


CONV_LDS_CFG0, CONV_LDS_NCFG = 16, 64  # csrc/kernels.h: LDS-staged conv configs (conv_lds.hip)
CONV_DEEP_CFG0, CONV_DEEP_NCFG = 128, 14  # conv_igemm tiles 0-13 at register-pipeline depth 4 (conv.hip)
LDS_TILES = [(64, 64), (128, 64), (64, 128), (128, 128), (32, 64), (64, 32), (32, 32), (128, 16)]
CONV_GLDS_CFG0, CONV_GLDS_NCFG = 160, 32  # LDS-DMA conv configs (conv_lds.hip conv_glds_kernel)
GLDS_TILES = [(64, 64), (128, 64), (64, 128), (128, 128), (256, 64), (128, 32), (256, 128), (64, 32)]
CONV_PATCH_CFG0, CONV_PATCH_NCFG = 192, 15  # 3x3 / stride-1 patch conv configs (conv_lds.hip conv_patch_kernel)
PATCH_TILES = [(256, 16), (256, 32), (256, 64), (128, 32), (128, 64)]  # strip capacity (pixels) x BN channels
PATCH_CB = [16, 32, 64]  # channel slice staged per pass
CONV_GDEEP_CFG0, CONV_GDEEP_NCFG = 208, 32  # LDS-DMA configs with a deep ring (up to 8 K chunks in flight)
CONV_PATCHP_CFG0, CONV_PATCHP_NCFG = 240, 15  # persistent, DMA-pipelined patch conv (one channel slice)
GDEEP_TILES = [0, 1, 2, 3, 5, 7]  # GLDS_TILES entries that have a deep ring (conv_lds.hip GL_NST_DEEP)
CONV_XCD = 4096  # flag on any conv config: XCD-contiguous tile order (csrc/common.h block_coords)


def lds_cfg(tile: int, kc: int = 64, splits: int = 1) -> int:
    """Config id of the LDS-staged conv kernel: tile index into LDS_TILES (BM pixels x BN channels), K chunk
    64 / 128, cross-block split of K into 1 / 2 / 4 / 8."""
    return CONV_LDS_CFG0 + 8 * tile + 4 * (kc == 128) + {1: 0, 2: 1, 4: 2, 8: 3}[splits]


def glds_cfg(tile: int, splits: int = 1, deep: bool = False) -> int:
    """Config id of the LDS-DMA conv kernel: tile index into GLDS_TILES (BM pixels x BN channels, K chunk 64,
    3-stage ring, or with ``deep`` the tile's deepest ring), cross-block split of K into 1 / 2 / 4 / 8."""
    return (CONV_GDEEP_CFG0 if deep else CONV_GLDS_CFG0) + 4 * tile + {1: 0, 2: 1, 4: 2, 8: 3}[splits]


def patch_cfg(tile: int, cb: int, persistent: bool = False) -> int:
    """Config id of the patch conv kernel: tile index into PATCH_TILES (a block owns R = BM // Wout whole
    output rows x BN channels), channel slice cb (16 / 32 / 64; Cs must be a multiple).  ``persistent``: the
    block loops over strips with the next one in flight by LDS-DMA (Cs == cb, no normalise-on-load)."""
    return (CONV_PATCHP_CFG0 if persistent else CONV_PATCH_CFG0) + 3 * tile + PATCH_CB.index(cb)


def conv_workspace(mode: int, cfg: int, G: int, d: dict, device) -> Optional[tuple]:
    """Attach the split-K workspace an LDS-staged conv config needs (fp32 partial tiles + zeroed arrival
    tickets) to the argument dict ``d``; returns the tensors to keep alive, or None when ``cfg`` cannot run
    these arguments."""
    if (cfg & ~CONV_XCD) < CONV_LDS_CFG0:
        return ()
    rc, ws, nt = lib().conv_workspace(mode, cfg, G, d)
    if rc != 0:
        return None
    if ws == 0:
        d.pop("ws", None)
        d.pop("cnt", None)
        return ()
    from ..engine import guard
    w = guard.alloc(ws, torch.float32, device, label=f"split-K workspace cfg {cfg}")
    c = guard.alloc(nt, torch.int32, device, zero=True, label=f"split-K tickets cfg {cfg}")
    d["ws"], d["cnt"] = w.data_ptr(), c.data_ptr()
    return (w, c)


class ConvCall:
    """A prepared convolution launch (packed weights + argument dict); ``run()`` enqueues it again."""

    def __init__(self, mode, cfg, d, out, keep, G=1):
        self.mode, self.cfg, self.d, self.out, self._keep, self.G = mode, cfg, d, out, keep, G
        ws = conv_workspace(mode, cfg, G, d, out.device)  # partial tiles and tickets of all G groups
        if ws is None:
            raise ValueError(f"conv config {cfg} cannot run this geometry")
        self._ws = ws

    def run(self):
        lib().conv(self.mode, self.cfg, self.G, stream(), self.d)
        return self.out


class WgradCall:
    def __init__(self, cfg, d, slab, post, keep):
        self.cfg, self.d, self.slab, self.post, self._keep = cfg, d, slab, post, keep

    def run(self):
        lib().wgrad(self.cfg, 1, stream(), self.d)
        return self.post(self.slab)


def prepare_conv2d(x, w, bias=None, stride=1, padding=0, stats=None, x2=None, cfg=None, nol=None, groups=None,
                   out=None, stats_nrep=None) -> ConvCall:
    """The forward launch of :func:`conv2d`.  ``x`` / ``x2`` may each be the column slice of a wider buffer (a pitched
    input).  ``out``: the bf16 output to write instead of a new one, possibly the column slice of a wider (concat)
    buffer.  ``stats_nrep``: replica rows in use of ``stats`` (a launch adds into row block % stats_nrep).
    ``groups`` = G: ``x``, ``x2``, ``w``, ``out`` carry a leading ``[G]`` dimension (the groups of ``x`` / ``out`` one
    stride apart), ``bias`` is ``[G, Co]`` and ``stats`` ``[G, NREP, 2, Co]``."""
    G = groups or 1
    lead = 1 if groups else 0
    if stats is not None and stats.dtype != torch.float64:
        raise TypeError("BN statistic replicas are fp64 ([NREP, 2, Co])")
    if not x.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"expected {torch.bfloat16}, got {x.dtype}")
    if x.dim() != 4 + lead or w.dim() != 4 + lead or (lead and (x.shape[0] != G or w.shape[0] != G)):
        raise ValueError("conv: x [(G,) B, H, W, C] and w [(G,) Co, Ci, KH, KW] expected")
    ld0, gs0 = _rows(x, lead, "x")
    C0 = x.shape[-1]
    C1 = x2.shape[-1] if x2 is not None else 0
    Cs = C0 + C1
    B, H, W, Co, Ci, KH, KW, sh, sw, ph, pw, Ho, Wo = _geom(x.shape[lead:], w.shape[lead:], stride, padding)
    if Ci > Cs:
        raise ValueError("weight has more input channels than the input")
    if lead:
        wf = torch.stack([pack_weight_fwd(w[z].float(), Cs) for z in range(G)])
    else:
        wf = pack_weight_fwd(w.float(), Cs)
    from ..engine import guard
    oshape = tuple(x.shape[:lead]) + (B, Ho, Wo, Co)
    if out is None:
        y = guard.alloc(oshape, torch.bfloat16, x.device, label=f"conv out cfg {cfg}")
    else:
        y = out
        if tuple(y.shape) != oshape:
            raise ValueError(f"out must be {oshape}")
    ldo, ogs = _rows(y, lead, "out")
    src = {"p0": ptr(x), "ld0": ld0, "gs0": gs0, "C0": C0, "C1": C1}
    if x2 is not None:
        if tuple(x2.shape[:-1]) != tuple(x.shape[:-1]):
            raise ValueError("x2 must have x's pixels")
        ld1, gs1 = _rows(x2, lead, "x2")
        src.update({"p1": ptr(x2), "ld1": ld1, "gs1": gs1})
    if bias is not None and lead and tuple(bias.shape) != (G, Co):
        raise ValueError("grouped bias must be [G, Co]")
    d = {"src": src, "w": ptr(wf), "wgs": wf.shape[-2] * wf.shape[-1] if lead else 0,
         "bias": ptr(bias) if bias is not None else 0, "bgs": Co if lead else 0, "out": ptr(y), "ldo": ldo, "ogs": ogs,
         "stats": ptr(stats) if stats is not None else 0, "B": B, "Hs": H, "Ws": W, "Ho": Ho, "Wo": Wo, "N": Co,
         "Npad": wf.shape[-2], "Cs": Cs, "KH": KH, "KW": KW, "sh": sh, "sw": sw, "ph": ph, "pw": pw,
         "Kpad": wf.shape[-1]}
    if stats_nrep is not None:
        d["stats_nrep"] = stats_nrep
    if nol is not None:  # (bn dict of x's BN, kind): x is a pre-BN y, the operand is act(BN(x)) on load
        d["nol"] = {"bn": nol[0], "kind": nol[1]}
    return ConvCall(0, _fwd_cfg(Co, B * Ho * Wo) if cfg is None else cfg, d, y, (x, x2, wf, bias, stats, nol), G)


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride=1, padding=0,
           stats: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None, cfg: Optional[int] = None,
           nol=None):
    """NHWC bf16 convolution.  ``x2`` (optional) is a second input whose channels are concatenated after
    ``x``'s (the kernel reads both without materialising the concat).  ``stats`` ([NREP, 2, Co] fp64,
    zero-initialised by the caller) receives per-channel sums of the output and its square.  ``nol``
    ((bn dict, kind)): normalise-on-load -- ``x`` is a pre-BN tensor and the conv input is act(BN(x))."""
    return prepare_conv2d(x, w, bias, stride, padding, stats, x2, cfg, nol).run()


def _rows(t: torch.Tensor, lead: int, what: str) -> Tuple[int, int]:
    """(pitch, group stride) of a bf16 ``[(G,) B, H, W, C]`` tensor read as rows of pixels: contiguous, or the
    column slice of a wider contiguous buffer (pitch = the buffer's channel count).  ``lead``: 1 if the tensor
    carries the group dimension."""
    if not t.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if t.dtype != torch.bfloat16 or t.dim() != 4 + lead or t.stride(-1) != 1:
        raise ValueError(f"{what}: expected a bf16 [{'G, ' if lead else ''}B, H, W, C] tensor with unit channel stride")
    ld = t.stride(-2)
    if t.stride(-3) != t.shape[-2] * ld or t.stride(-4) != t.shape[-3] * t.shape[-2] * ld:
        raise ValueError(f"{what}: the pixels must be rows of one pitch")
    return ld, (t.stride(0) if lead else 0)


def prepare_conv2d_dgrad(dy, w, in_hw, stride=1, padding=0, cin_stored=None, cfg=None, bn_stats=None, groups=None,
                         add=None, out=None) -> ConvCall:
    """``dy`` may be the column slice of a wider buffer (a branch conv's share of a concat gradient).  ``out``: the
    bf16 ``[(G,) B, H, W, Cin_stored]`` gradient to write instead of a new one, possibly the column slice of a wider
    buffer (the groups of ``dy`` / ``out`` one stride apart).
    ``bn_stats`` (optional): ``(y, bn, part, kind)`` -- the dgrad output is the gradient of
    ``act(BN(y))`` and the epilogue accumulates that BN's backward sums sum(dz), sum(dz*xhat) into rows 0/1
    of ``part`` ([NREP, 3, C] fp64, zero-initialised); see :func:`bn_tail_backward` ``stats_done``.  Or a dict
    with those four keys and optionally ``r`` (ADD_RELU: the residual), ``bn2`` (its BN: projection shortcut, row
    2 of ``part`` receives sum(dz*xhat2)), ``C`` (the tail's channels when the gradient has more: ``y`` / ``r``
    are ``C`` wide) and ``pgs`` (group stride of ``part``; 0: every group adds into one shared tail, ``y`` /
    ``r`` then carry no group dimension).
    ``add``: up to 3 more bf16 gradient sources of the output's shape, summed in the epilogue before its one
    rounding; each may be a column slice of a wider buffer.
    ``groups`` = G: ``dy``, ``w``, the sources, ``y`` / ``r`` and the output carry a leading ``[G]`` dimension,
    ``part`` is ``[G, NREP, 3, C]`` and the BN parameters ``[G, C]`` (:func:`bn_args`)."""
    G = groups or 1
    lead = 1 if groups else 0
    if not dy.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if dy.dtype != torch.bfloat16:
        raise TypeError(f"expected {torch.bfloat16}, got {dy.dtype}")
    if dy.dim() != 4 + lead or w.dim() != 4 + lead or (lead and (dy.shape[0] != G or w.shape[0] != G)):
        raise ValueError("dgrad: dy [(G,) B, Ho, Wo, Co] and w [(G,) Co, Ci, KH, KW] expected")
    ld0, gs0 = _rows(dy, lead, "dy")
    B, Ho, Wo, Co = dy.shape[lead:]
    _, Ci, KH, KW = w.shape[lead:]
    Cs = cin_stored or Ci
    H, W = in_hw
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    if lead:
        wd = torch.stack([pack_weight_dgrad(w[z].float(), Cs) for z in range(G)])
    else:
        wd = pack_weight_dgrad(w.float(), Cs)
    from ..engine import guard
    oshape = ((G,) if lead else ()) + (B, H, W, Cs)
    if out is None:
        dx = guard.alloc(oshape, torch.bfloat16, dy.device, label=f"dgrad out cfg {cfg}")
    else:
        dx = out
        if tuple(dx.shape) != oshape:
            raise ValueError(f"out must be {oshape}")
    ldo, ogs = _rows(dx, lead, "out")
    d = {"src": {"p0": ptr(dy), "ld0": ld0, "C0": Co, "C1": 0, "gs0": gs0},
         "w": ptr(wd), "wgs": wd.shape[-2] * wd.shape[-1] if lead else 0, "out": ptr(dx), "ldo": ldo, "ogs": ogs,
         "B": B, "Hs": Ho, "Ws": Wo, "Ho": H, "Wo": W, "N": Cs, "Npad": wd.shape[-2], "Cs": Co, "KH": KH, "KW": KW,
         "sh": sh, "sw": sw, "ph": ph, "pw": pw, "Kpad": wd.shape[-1]}
    keep = (dy, wd)
    if add:
        srcs = []
        for t in add:
            if tuple(t.shape) != tuple(dx.shape):
                raise ValueError("add: every extra gradient source has the output's shape")
            ld, gs = _rows(t, lead, "add")
            srcs.append({"p": ptr(t), "ld": ld, "gs": gs})
        d["add"] = srcs
        keep = keep + tuple(add)
    if bn_stats is not None:
        if not isinstance(bn_stats, dict):
            y, bn, part, kind = bn_stats
            bn_stats = {"y": y, "bn": bn, "part": part, "kind": kind}
        y, bn, part, kind = bn_stats["y"], bn_stats["bn"], bn_stats["part"], bn_stats["kind"]
        r, bn2, pgs = bn_stats.get("r"), bn_stats.get("bn2"), bn_stats.get("pgs")
        C = bn_stats.get("C") or Cs
        ylead = 0 if pgs == 0 else lead  # one shared tail: y / r have no group dimension
        if part.dtype != torch.float64 or tuple(y.shape[-4:]) != (B, H, W, C) or y.dim() != 4 + ylead:
            raise ValueError("bn_stats: y must be the [B, H, W, C] bf16 BN input and part fp64 [NREP, 3, C]")
        ldy, ygs = _rows(y, ylead, "bn_stats y")
        b = {"y": ptr(y), "ldy": ldy, "ygs": ygs, "bn": bn, "part": ptr(part), "kind": kind, "C": C}
        if pgs is not None:
            b["pgs"] = pgs
        if r is not None:
            if tuple(r.shape) != tuple(y.shape):
                raise ValueError("bn_stats: r must have y's shape")
            ldr, rgs = _rows(r, ylead, "bn_stats r")
            b.update({"r": ptr(r), "ldr": ldr, "rgs": rgs})
        if bn2 is not None:
            b["bn2"] = bn2
        d["bnb"] = b
        keep = keep + (y, part, r)
    return ConvCall(1, _fwd_cfg(Cs, B * H * W) if cfg is None else cfg, d, dx, keep, G)


def conv2d_dgrad(dy: torch.Tensor, w: torch.Tensor, in_hw: Tuple[int, int], stride=1, padding=0,
                 cin_stored: Optional[int] = None, cfg: Optional[int] = None, bn_stats=None, groups=None, add=None,
                 out: Optional[torch.Tensor] = None):
    """Gradient w.r.t. the NHWC input: bf16 ``[B, H, W, Cin_stored]`` (fp32 accumulation, one rounding)."""
    return prepare_conv2d_dgrad(dy, w, in_hw, stride, padding, cin_stored, cfg, bn_stats, groups, add, out).run()


# Weight-gradient tile configurations: the Python copy of csrc/wgrad_tile.h WGRAD_CONFIGS (the package imports and
# lowers programs where the extension is absent; tests/test_wgrad_configs.py holds the two equal row by row).
# im2col families: TN output channels x TK reduction columns, MCH pixels per LDS chunk; patch: TN x 9 taps x CB
# input channels, W8 = max padded output width, R = output rows per strip.
WgradCfg = namedtuple("WgradCfg", "family TN TK MCH CB W8 R", defaults=(0, 0, 0, 0, 0))
WGRAD_FAMILIES = ("small", "whole", "patch", "big", "lean", "leanbig")  # csrc/wgrad_tile.h WgFamily, in its order


def _cfgs(family, cfg0, fields, *rows):
    return {cfg0 + i: WgradCfg(family, **dict(zip(fields, r))) for i, r in enumerate(rows)}


_IM2COL, _PATCH = ("TN", "TK", "MCH"), ("TN", "CB", "W8", "R")
WGRAD_CONFIGS = {
    **_cfgs("small", 0, _IM2COL, (16, 32, 128), (32, 32, 128), (32, 64, 64), (64, 64, 64), (16, 64, 128),
            (16, 32, 256), (32, 32, 256), (64, 32, 64)),
    # whole-reduction tiles for small-Cout layers
    **_cfgs("whole", 8, _IM2COL, (16, 192, 64), (16, 128, 64), (32, 192, 64), (32, 320, 32)),
    # 3x3 / stride-1 patch kernels, padding 1 or 0 (csrc/conv.hip WgPatch::run)
    **_cfgs("patch", 12, _PATCH, (16, 16, 88, 4), (32, 16, 88, 4), (32, 32, 48, 4), (64, 32, 24, 4),
            (32, 32, 128, 2), (64, 32, 128, 2), (64, 16, 128, 2), (32, 16, 128, 2)),
    # large tiles on the 32x32x16 MFMA (csrc/conv.hip wgrad_big_block); their last K tile may be partial
    **_cfgs("big", 32, _IM2COL, (64, 64, 64), (64, 128, 64), (128, 64, 64), (128, 128, 64)),
    # lean-staging im2col tiles (csrc/wgrad_lean.hip: per-chunk pixel table in LDS, per-thread staging constants,
    # branch-free loads; their own M split: engine/core.py wgrad_plan); partial last K tile
    **_cfgs("lean", 36, _IM2COL, (16, 64, 256), (16, 144, 128), (32, 64, 256), (32, 144, 128), (64, 64, 128),
            (64, 128, 128), (128, 64, 128), (128, 128, 64)),
    # the same staging under the large tiles' 32x32x16 MFMA compute and M split (wgrad_lean_twin)
    **_cfgs("leanbig", 44, _IM2COL, (64, 64, 64), (64, 128, 64), (128, 64, 64), (128, 128, 64)),
}
WGRAD_TILES = {c: (v.TN, v.TK, v.MCH) for c, v in WGRAD_CONFIGS.items() if v.family != "patch"}
WGRAD_PATCH = {c: (v.TN, v.CB, v.W8, v.R) for c, v in WGRAD_CONFIGS.items() if v.family == "patch"}


def wgrad_family(cfg: int) -> str:
    return WGRAD_CONFIGS[cfg].family


def wgrad_big_cfg(Npad: int, Kpad: int) -> int:
    """The large tile a conv's shape suits: 128 rows when Cout fills them, 128 columns when the reduction does."""
    return 32 + 2 * (Npad > 64) + (Kpad > 64)


def wgrad_lean_twin(cfg: int) -> int:
    """The lean-staging form of a large-tile config (same tile, same M split); any other config is its own."""
    return cfg + 12 if wgrad_family(cfg) == "big" else cfg


def wgrad_ktiles(cfg: int, Kpad: int) -> int:
    """K tiles of an im2col weight-gradient config over a padded reduction of ``Kpad`` columns; 0 if the
    config cannot cover it (the small-tile kernels need TK | Kpad)."""
    c = WGRAD_CONFIGS[cfg]
    if c.family in ("small", "whole"):
        return 0 if Kpad % c.TK else Kpad // c.TK
    return math.ceil(Kpad / c.TK)


def patch_valid(cfg, Cs, KH, KW, stride, padding, Hi, Wi, Ho, Wo, C0=None, C1=0) -> bool:
    TN, CB, W8, R = WGRAD_PATCH[cfg]
    s = (stride, stride) if isinstance(stride, int) else tuple(stride)
    p = (padding, padding) if isinstance(padding, int) else tuple(padding)
    return ((KH, KW) == (3, 3) and s == (1, 1) and p[0] in (0, 1) and p[1] in (0, 1)
            and (Ho, Wo) == (Hi + 2 * p[0] - 2, Wi + 2 * p[1] - 2) and Cs % CB == 0
            and _pad(Wo, 8) <= W8 and (R * _pad(Wo, 8)) % 32 == 0 and (C1 == 0 or C0 % CB == 0))


KG_CH_BITS, KG_TAP_BITS = 14, 7  # csrc/conv_tile.h encode_kg: channel offset within a segment, tap index


def wgrad_ntiles(cfg: int, d: dict) -> int:
    """csrc/conv.hip wgrad_ntiles on the argument dict of a weight-gradient launch (geometry and pitches only):
    tiles per group, -1 no such config, -2 the config cannot take this conv -- its tiles do not cover it, or a
    value its kernel packs into a bit field or a 32-bit offset would not fit."""
    c = WGRAD_CONFIGS.get(cfg)
    if c is None:
        return -1
    src, Cs, Kpad, KH, KW = d["src"], d["Cs"], d["Kpad"], d["KH"], d["KW"]
    C0, C1 = src.get("C0", 0), src.get("C1", 0)
    rows = math.ceil(d["Npad"] / c.TN)
    if c.family == "patch":
        ok = patch_valid(cfg, Cs, KH, KW, (d["sh"], d["sw"]), (d["ph"], d["pw"]), d["Hi"], d["Wi"], d["Ho"], d["Wo"],
                         C0, C1) and Kpad >= 9 * Cs
        return rows * (Cs // c.CB) if ok else -2
    w0 = min(C0, Cs)  # encode_kg: offsets below w0 in segment 0, below Cs - w0 in segment 1; taps below KH, KW
    if max(w0, Cs - w0) - 8 >= 1 << KG_CH_BITS or max(KH, KW) - 1 >= 1 << KG_TAP_BITS:
        return -2
    if c.family in ("lean", "leanbig"):
        M, xin = d["B"] * d["Ho"] * d["Wo"], d["B"] * d["Hi"] * d["Wi"]
        ld = max(src["ld0"], src.get("ld1", src["ld0"]) if C1 > 0 else 0)
        if not (M < 1 << 24 and xin * ld < 1 << 31 and M * d["ldd"] < 1 << 31 and d["Wi"] < 32768 and d["Hi"] < 16384
                and KH < 128 and KW < 128 and rows * c.TN - 8 < 1 << KG_CH_BITS):
            return -2
    return rows * wgrad_ktiles(cfg, Kpad) or -2


def patch_plan(cfg, B, Ho, Npad, Cs, G=1, target=512):
    """(splits, units per split) of a patch wgrad: unit = (image, strip of R output rows).  (Capping the
    units per block at 3 to even out the blocks of a batched launch measured 4 % slower on Model A: the
    extra splits cost more slab traffic in the finalize than the shorter blocks saved.)"""
    TN, CB, _, R = WGRAD_PATCH[cfg]
    U = B * math.ceil(Ho / R)
    tiles = math.ceil(Npad / TN) * (Cs // CB) * G
    splits = max(1, min(U, math.ceil(target / tiles)))
    ups = math.ceil(U / splits)
    return math.ceil(U / ups), ups


def wgrad_cfg(Co: int, Kpad: int) -> int:
    return 0 if Co <= 16 else ((1 if Kpad <= 64 else 2) if Co <= 32 else 3)


def prepare_conv2d_wgrad(x, dy, w_shape, stride=1, padding=0, x2=None, splits=None, cfg=None, nol=None) -> WgradCall:
    _check(x, torch.bfloat16)
    _check(dy, torch.bfloat16)
    Co, Ci, KH, KW = w_shape
    C1 = x2.shape[-1] if x2 is not None else 0
    Cs = x.shape[-1] + C1
    B, H, W, _ = x.shape
    _, Ho, Wo, _ = dy.shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    Kpad = _pad(KH * KW * Cs, 64)
    Npad = _pad(Co, 16)
    if cfg is None:
        cfg = wgrad_cfg(Co, Kpad)
    src = {"p0": ptr(x), "ld0": x.shape[-1], "C0": x.shape[-1], "C1": C1}
    if x2 is not None:
        src.update({"p1": ptr(x2), "ld1": C1})
    d = {"src": src, "dy": ptr(dy), "ldd": Co, "B": B, "Hi": H, "Wi": W, "Ho": Ho, "Wo": Wo, "Co": Co, "Npad": Npad,
         "Cs": Cs, "KH": KH, "KW": KW, "sh": sh, "sw": sw, "ph": ph, "pw": pw, "Kpad": Kpad}
    tiles = wgrad_ntiles(cfg, d)
    if tiles < 0:
        raise ValueError(f"wgrad config {cfg} {WGRAD_CONFIGS.get(cfg)} does not fit this convolution (Kpad {Kpad})")
    if wgrad_family(cfg) == "patch":
        splits, mps = patch_plan(cfg, B, Ho, Npad, Cs)
    else:
        MCH = WGRAD_CONFIGS[cfg].MCH
        M = B * Ho * Wo
        if splits is None:
            splits = max(1, min(math.ceil(M / MCH), math.ceil(512 / tiles)))
        mps = _pad(math.ceil(M / splits), MCH)
        splits = math.ceil(M / mps)
    from ..engine import guard
    slab = guard.alloc((1, splits, Npad, Kpad), torch.float32, x.device, label=f"wgrad slab cfg {cfg}")
    d.update(slab=ptr(slab), splits=splits, m_per_split=mps)

    if nol is not None:  # (consts [1, 4, Cs] fp32: scale, shift, mean, invstd; kind)
        d["nol"] = {"consts": ptr(nol[0]), "kind": nol[1]}

    def post(sl):
        dWp = sl.sum(dim=1)[0, :Co, :KH * KW * Cs].view(Co, KH, KW, Cs)[..., :Ci]
        return dWp.permute(0, 3, 1, 2).contiguous()
    return WgradCall(cfg, d, slab, post, (x, x2, dy, nol))


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, w_shape, stride=1, padding=0, x2: Optional[torch.Tensor] = None,
                 splits: Optional[int] = None, cfg: Optional[int] = None, nol=None):
    """Weight gradient in the reference layout ``[Co, Ci, KH, KW]`` (fp32).  ``nol`` ((consts, kind)): ``x``
    is pre-BN and the operand is act(x * consts[0,0] + consts[0,1]), as in a normalise-on-load forward."""
    return prepare_conv2d_wgrad(x, dy, w_shape, stride, padding, x2, splits, cfg, nol).run()


# ---------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_SIGMOID, SIGMUL, ADD_RELU, POOL_RELU = range(6)


def bn_args(stats, gamma, beta, run_mean, run_var, nbt, count, eps=1e-5, momentum=0.1, training=True,
            consts=None, nrep=None, pnrep=None, sld=None, coff=0):
    """Kernel BN descriptor.  The dict keeps references to the tensors it points at (``_keep``) so that
    they cannot be freed while a launch may still use them.  Grouped launches: parameters ``[G, C]``, ``stats``
    ``[G, NREP, 2, C]``.  ``consts`` ([G, 4, C] fp32: scale, shift, mean, invstd): the batch constants the
    forward tail publishes and every backward kernel reads instead of the replicas; ``nrep`` / ``pnrep``:
    replicas in use of the forward sums / of the backward partial sums (powers of two <= NREP).  ``sld`` / ``coff``:
    this BN's channels are columns [coff, coff + C) of replica rows ``sld`` wide (``stats`` [G, NREP, 2, sld]: the
    combined rows of a conv whose output channels feed several BNs)."""
    if stats.dtype != torch.float64:
        raise TypeError("BN statistic replicas are fp64 ([NREP, 2, C])")
    if gamma.dim() == 2 and not all(t.is_contiguous() and t.shape == gamma.shape for t in (gamma, beta, run_mean, run_var)):
        raise ValueError("grouped BN parameters must be contiguous [G, C]")
    d = {"_keep": (stats, gamma, beta, run_mean, run_var, nbt, consts), "stats": ptr(stats, coff),
         "gamma": ptr(gamma), "beta": ptr(beta), "run_mean": ptr(run_mean),
         "run_var": ptr(run_var), "nbt": ptr(nbt) if nbt is not None else 0,
         "pstride": gamma.shape[-1] if gamma.dim() == 2 else 0, "C": gamma.shape[-1],
         "count": count, "eps": eps, "momentum": momentum, "training": 1 if training else 0}
    if consts is not None:
        _check(consts, torch.float32)
        if tuple(consts.shape[-2:]) != (4, gamma.shape[-1]):
            raise ValueError("consts must be [G, 4, C]")
        d["consts"] = ptr(consts)
    if nrep is not None:
        d["nrep"] = nrep
    if pnrep is not None:
        d["pnrep"] = pnrep
    if sld is not None:
        d["sld"] = sld
    return d


def tail_fwd_args(kind: int, y: torch.Tensor, bn: dict, r: Optional[torch.Tensor] = None, bn2: Optional[dict] = None,
                  groups: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """(argument dict, output) of a forward tail launch (:func:`bn_tail`; a job of ``lib().tail_table``)."""
    lead = 1 if groups else 0
    B, H, W, C = y.shape[lead:]
    oshape = tuple(y.shape[:lead]) + ((B, (H + 1) // 2, (W + 1) // 2, C) if kind == POOL_RELU else (B, H, W, C))
    if out is None:
        out = torch.empty(oshape, device=y.device, dtype=torch.bfloat16)
    elif tuple(out.shape) != oshape:
        raise ValueError(f"out must be {oshape}")
    ldy, ygs = _rows(y, lead, "y")
    ldo, ogs = _rows(out, lead, "out")
    d = {"y": ptr(y), "ldy": ldy, "ygs": ygs, "bn": bn, "out": ptr(out), "ldo": ldo,
         "ogs": ogs, "B": B, "H": H, "W": W, "C": C}
    if r is not None:
        ldr, rgs = _rows(r, lead, "r")
        d.update({"r": ptr(r), "ldr": ldr, "rgs": rgs})
    if bn2 is not None:
        d["bn2"] = bn2
    return d, out


def bn_tail(kind: int, y: torch.Tensor, bn: dict, r: Optional[torch.Tensor] = None, bn2: Optional[dict] = None,
            blocks: int = 64, groups: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """Fused BN(+act/+mul/+residual/+pool) forward on NHWC bf16 ``y``; returns the bf16 output.  ``groups`` = G:
    ``y`` / ``r`` and the output carry a leading ``[G]`` dimension (BN parameters ``[G, C]``).  ``y``, ``r`` and
    ``out`` (the output to write instead of a new one) may each be the column slice of a wider buffer."""
    d, out = tail_fwd_args(kind, y, bn, r, bn2, groups, out)
    lib().tail_fwd(kind, groups or 1, blocks, stream(), d)
    return out


def bnb_cgb(C: int) -> int:
    """Channel groups of 8 per block of the 2-D tiled BN backward (csrc/bn.hip bnb_cgb)."""
    cg = C // 8
    for g in (8, 4, 2):
        if cg % g == 0:
            return g
    return 1


def bnb_plan(M: int, C: int, G: int = 1, target_blocks: int = 1024):
    """Chunking of the 2-D tiled BN backward (csrc/bn.hip bnb_*): blocks of 256 threads cover 8*CGB
    channels x 256/CGB pixel lanes; chunks are sized so that chunks x channel blocks x G ~ target_blocks
    (at most 8 pixel steps per thread).  Returns (nchunk, pixels per chunk)."""
    cgb = bnb_cgb(C)
    pl = 256 // cgb
    steps = max(1, math.ceil(M / pl))
    cblocks = (C // (8 * cgb)) * G
    per = max(1, min(8, math.ceil(steps * cblocks / target_blocks)))
    chunk_px = pl * per
    return math.ceil(M / chunk_px), chunk_px


def bn_tail_backward(kind: int, y: torch.Tensor, bn: dict, grads: Sequence[torch.Tensor], dgamma, dbeta,
                     r: Optional[torch.Tensor] = None, bn2: Optional[dict] = None, dgamma2=None, dbeta2=None,
                     fused=False, store_dz: bool = False, part: Optional[torch.Tensor] = None,
                     gscale: float = 1.0, groups: Optional[int] = None, out: Optional[dict] = None):
    """Returns ``(dy bf16, side bf16 | None, dy2 bf16 | None)``; writes dgamma/dbeta (and 2) in place.
    ``grads``: the upstream gradient sources (bf16, as the engine stores them; other dtypes are rounded), each
    possibly a column slice of a wider buffer;
    ``fused``: 1 / True = single-launch variant (block per 8 channels over all pixels) instead of reduce + apply;
    3 = reduce only: the statistics of ``grads`` (a subset of the tail's sources) are added into ``part``, nothing
    else is written and ``(None, None, None)`` is returned (dgamma / dbeta are not used);
    ``store_dz``: the reduce stores dz and the apply reads it instead of recomputing it;
    ``part``: the statistics were already accumulated (by a dgrad with ``bn_stats``, by ``fused=3`` launches):
    apply pass only (``fused=2``);
    ``gscale``: factor on the dgamma / dbeta the apply writes;
    ``groups`` = G: every tensor carries a leading ``[G]`` dimension (``part`` [G, NREP, 3, C], parameters and
    their gradients [G, C]);
    ``out``: preallocated contiguous bf16 outputs of y's shape to write instead of new ones (keys ``dy``, ``side``,
    ``dy2``)."""
    G = groups or 1
    lead = 1 if groups else 0
    B, H, W, C = y.shape[lead:]
    lshape = tuple(y.shape[:lead])
    nchunk, chunk_px = bnb_plan(B * H * W, C, G)
    mode = int(fused)
    if mode == 3:
        if part is None:
            raise ValueError("fused=3 adds the sources' statistics into part")
    elif part is not None:
        mode = 2
    else:
        part = torch.zeros(lshape + (NREP, 3, C), device=y.device, dtype=torch.float64)
    grads = [g if (g.is_cuda and g.dtype == torch.bfloat16 and g.stride(-1) == 1) else _grad(g) for g in grads]
    ldy, ygs = _rows(y, lead, "y")
    d = {"y": ptr(y), "ldy": ldy, "ygs": ygs, "bn": bn, "B": B, "H": H, "W": W, "C": C,
         "g": [(ptr(g),) + _rows(g, lead, "grads")[::-1] for g in grads], "part": ptr(part), "chunk_px": chunk_px,
         "fused": mode, "gscale": gscale}
    if r is not None:
        ldr, rgs = _rows(r, lead, "r")
        d.update({"r": ptr(r), "ldr": ldr, "rgs": rgs})
    if bn2 is not None:
        d["bn2"] = bn2
    if mode == 3:
        lib().tail_bwd(kind, G, nchunk, stream(), d)
        return None, None, None
    px = B * H * W * C

    def _out(name):
        t = (out or {}).get(name)
        if t is None:
            return torch.empty(tuple(y.shape), device=y.device, dtype=torch.bfloat16)
        _check(t, torch.bfloat16)
        if t.shape != y.shape:
            raise ValueError(f"out[{name!r}] must have y's shape")
        return t
    dy = _out("dy")
    d.update({"dy": ptr(dy), "ldd": C, "dgs": px if lead else 0, "dgamma": ptr(dgamma), "dbeta": ptr(dbeta),
              "pgs": C if lead else 0})
    dzbuf = None
    if store_dz:
        dzbuf = torch.empty(tuple(y.shape), device=y.device, dtype=torch.bfloat16)
        d.update({"dzbuf": ptr(dzbuf), "lddz": C, "dzgs": px if lead else 0})
    side = dy2 = None
    if kind in (SIGMUL,) or (kind == ADD_RELU and bn2 is None):
        side = _out("side")
        d.update({"side": ptr(side), "lds": C, "sgs": px if lead else 0})
    if bn2 is not None:
        dy2 = _out("dy2")
        d.update({"dy2": ptr(dy2), "ldd2": C, "d2gs": px if lead else 0, "dgamma2": ptr(dgamma2),
                  "dbeta2": ptr(dbeta2)})
    lib().tail_bwd(kind, G, nchunk, stream(), d)
    return dy, side, dy2


def pool3(x: torch.Tensor, is_max: bool, am: Optional[torch.Tensor] = None):
    """Inception pools on NHWC bf16: max 3x3/s2 (valid) or avg 3x3/s1/p1 (count_include_pad).  ``am``
    (max only, uint8 [B, Ho, Wo, C]): receives each output's window argmax for :func:`pool3_backward`."""
    B, H, W, C = x.shape
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if is_max else (H, W)
    y = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.bfloat16)
    d = {"x": ptr(x), "ldx": C, "y": ptr(y), "ldy": C, "B": B, "H": H, "W": W, "C": C, "Ho": Ho, "Wo": Wo}
    if am is not None:
        if am.dtype != torch.uint8 or am.numel() != B * Ho * Wo * C:
            raise ValueError("am must be uint8 with one entry per output element")
        d["am"] = ptr(am)
    lib().pool3(int(is_max), 0, stream(), d)
    return y


def pool3_backward(x: torch.Tensor, g: torch.Tensor, is_max: bool, am: Optional[torch.Tensor] = None):
    """Input gradient (bf16) of :func:`pool3` from the output gradient ``g`` (bf16; other dtypes are rounded)."""
    B, H, W, C = x.shape
    _, Ho, Wo, _ = g.shape
    g = _grad(g)
    dx = torch.empty(B, H, W, C, device=x.device, dtype=torch.bfloat16)
    d = {"x": ptr(x), "ldx": C, "g": ptr(g), "ldg": C, "dx": ptr(dx), "lddx": C, "B": B, "H": H, "W": W, "C": C,
         "Ho": Ho, "Wo": Wo}
    if am is not None:  # the kernel reads the argmax with 8-byte loads per 8-channel group
        if am.dtype != torch.uint8 or am.numel() != B * Ho * Wo * C or C % 8 or not is_max:
            raise ValueError("am must be the uint8 [B, Ho, Wo, C] argmax of a max pool with C % 8 == 0")
        d["am"] = ptr(am)
    lib().pool3(int(is_max), 1, stream(), d)
    return dx


def gather_args(*, X, labels, lab_w: int, idx, out, lab_out, B: int, H: int, W: int, taps: int = 0, off: int = 0,
                zero=(), cursor=None, noise: Optional[dict] = None) -> dict:
    """The launch dict of the batch gather as the binding reads it, the one builder behind :func:`gather_batch`,
    :func:`gather_batch_noise` and the engine's gather phase.  The arguments are :func:`gather_batch`'s; ``out`` /
    ``lab_out``: the [B, H, W, 8] bf16 and [B, lab_w] int64 tensors written; ``zero``: (pointer, bytes) pairs.
    ``noise`` (:func:`noise_args`) is nested under ``"noise"``: the key selects the noisy kernel, absent the clean."""
    d = {"X": ptr(X), "idx": ptr(idx), "lab": ptr(labels), "lab_w": lab_w, "out": ptr(out), "lab_out": ptr(lab_out),
         "B": B, "Cin": X.shape[1], "H": H, "W": W, "taps": taps, "off": off, "zero": list(zero),
         "cursor": ptr(cursor), "nrows": idx.shape[0] if cursor is not None else 0}
    if noise is not None:
        d["noise"] = noise
    return d


def gather_batch(X: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, taps: int = 0, off: int = 0,
                 zero: Sequence[torch.Tensor] = (), cursor: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, noise: Optional[dict] = None):
    """HBM-resident dataset rows -> (bf16 NHWC batch with C padded to 8, labels).  ``idx``: int64 [B], or with
    ``cursor`` (a device int64 scalar) a [nrows, B] schedule whose row ``cursor`` mod nrows is gathered.  ``taps`` /
    ``off``: the 1-channel stem's vertical tap packing.  ``zero``: up to 4 tensors the launch clears (16-byte aligned
    and sized).  ``out``: the [B, H, W, 8] bf16 output to write.  ``noise``: :func:`noise_args` -- every real element
    becomes ``bf16(x + sigma * g)`` (:func:`gather_batch_noise`)."""
    _check(X, torch.float32)
    _check(idx, torch.int64)
    _check(labels, torch.int64)
    N, Cin, H, W = X.shape
    B = idx.shape[-1] if cursor is not None else idx.numel()
    if cursor is not None:
        _check(cursor, torch.int64)
        if idx.dim() != 2:
            raise ValueError("a cursor needs a [nrows, B] index schedule")
    if out is None:
        out = torch.empty(B, H, W, 8, device=X.device, dtype=torch.bfloat16)
    _check(out, torch.bfloat16)
    if out.numel() < B * H * W * 8:
        raise ValueError("output too small")
    lw = labels.shape[1] if labels.dim() == 2 else 1
    lab = torch.empty(B, lw, device=X.device, dtype=torch.int64)
    zero = [(z.data_ptr(), z.numel() * z.element_size()) for z in zero]
    lib().gather_batch(stream(), gather_args(X=X, labels=labels, lab_w=lw, idx=idx, out=out, lab_out=lab, B=B, H=H, W=W,
                                             taps=taps, off=off, zero=zero, cursor=cursor, noise=noise))
    return out, lab


def sample_power(X: torch.Tensor) -> torch.Tensor:
    """Mean power of every clean plane of a resident set: X [N, C, H, W] fp32 -> P [N, C] fp32, the mean over the
    plane of (x - mean(x))^2 (data/noise.py; two passes with fp64 accumulators)."""
    _check(X, torch.float32)
    if X.dim() != 4:
        raise ValueError("dataset must be [N, C, H, W]")
    N, C, H, W = X.shape
    P = torch.empty(N, C, device=X.device, dtype=torch.float32)
    lib().sample_power(ptr(X), ptr(P), N * C, H * W, stream())
    return P


def noise_args(power: torch.Tensor, snr: torch.Tensor, draw: torch.Tensor, seed: int, noise_stream: int) -> dict:
    """The noise inputs of the batch gather as the binding reads them, the ``"noise"`` dict nested in
    :func:`gather_args`: the device power table [N, C], the device (lo, hi) fp32 pair, the device int64 draw number,
    and the launch constants (seed, stream id).  The three tensors live where the dataset does (the callers check
    that: a program lowers on the CPU too)."""
    for t, dtype in ((power, torch.float32), (snr, torch.float32), (draw, torch.int64)):
        if t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"expected a contiguous {dtype} tensor, got {t.dtype}")
    if snr.numel() != 2 or draw.numel() != 1:
        raise ValueError("snr must hold (lo, hi) and draw one number")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return {"power": ptr(power), "snr": ptr(snr), "draw": ptr(draw), "seed_lo": seed & 0xFFFFFFFF,
            "seed_hi": seed >> 32, "noise_stream": int(noise_stream)}


def gather_batch_noise(X: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, power: torch.Tensor,
                       snr: torch.Tensor, draw: torch.Tensor, seed: int, noise_stream: int = 0, taps: int = 0,
                       off: int = 0, zero: Sequence[torch.Tensor] = (), cursor: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, dbg: Optional[torch.Tensor] = None):
    """:func:`gather_batch` with SNR noise (data/noise.py): every real element is ``bf16(x + sigma * g)``, padding
    channels and out-of-image taps stay 0.  ``power``: :func:`sample_power` of ``X``; ``snr``: device fp32 (lo, hi);
    ``draw``: device int64 scalar; ``noise_stream``: 0 training, 2 evaluation.  ``idx`` / ``cursor``, ``taps`` /
    ``off``, ``zero`` and ``out``: :func:`gather_batch`'s.  ``dbg``: an fp32 [B, Cin, H, W] tensor that receives the
    unrounded noisy values (test hook).  Returns (out, labels)."""
    N, Cin, H, W = X.shape
    if tuple(power.shape) != (N, Cin):
        raise ValueError(f"power table must be [{N}, {Cin}]")
    for t in (power, snr, draw):
        _check(t)
    d = noise_args(power, snr, draw, seed, noise_stream)
    if dbg is not None:
        _check(dbg, torch.float32)
        if dbg.numel() < (idx.shape[-1] if cursor is not None else idx.numel()) * Cin * H * W:
            raise ValueError("dbg too small")
        d["dbg"] = ptr(dbg)
    return gather_batch(X, labels, idx, taps=taps, off=off, zero=zero, cursor=cursor, out=out, noise=d)


def noise_advance(draw: torch.Tensor):
    """``draw += 1`` on the device (the launch a training gather phase appends after its noise gather)."""
    _check(draw, torch.int64)
    lib().noise_advance(ptr(draw), stream())


def _starts(s, device) -> torch.Tensor:
    """A window-start table as the kernels read it: int32 on the device."""
    return torch.as_tensor(s).to(device=device, dtype=torch.int32).contiguous()


def _gather_out(device, fs: torch.Tensor, window: Tuple[int, int], B: int, taps: int, off: int, lab_w: int):
    """What both window gathers write and share: the bf16 NHWC-8 batch, the labels, and the launch fields of the
    batch geometry (fiber starts, window, tap packing) and of the two outputs."""
    out = torch.empty(B, window[0], window[1], 8, device=device, dtype=torch.bfloat16)
    lab = torch.empty(B, lab_w, device=device, dtype=torch.int64)
    return ({"fs": ptr(fs), "nf": fs.numel(), "B": B, "Wf": window[0], "Wt": window[1], "taps": taps, "off": off,
             "out": ptr(out), "lab_out": ptr(lab), "lab_w": lab_w}, out, lab)


def _prob_source(src: torch.Tensor, K: int, ncls: Optional[Sequence[int]]):
    """The source of a probability launch checked against the table's ``K`` columns: the heads' log-probabilities
    [T, B, 16] with one ``ncls`` per task, or logits [B, K].  Returns ``B`` and the launch fields."""
    _check(src, torch.float32)
    if ncls is not None:
        if src.dim() != 3 or src.shape[2] != 16 or src.shape[0] != len(ncls):
            raise ValueError("log-probabilities must be [T, B, 16] with one ncls per task")
        B = src.shape[1]
    else:
        if src.dim() != 2 or src.shape[1] != K:
            raise ValueError("logits must be [B, K]")
        B = src.shape[0]
    d = {"B": B, "src": ptr(src), "softmax": int(ncls is None), "K": K}
    if ncls is not None:
        d["ncls"] = [int(k) for k in ncls]
    return B, d


def selection_args(sel: Optional[torch.Tensor], count: Optional[torch.Tensor], idx, cursor,
                   live: bool = False) -> dict:
    """The launch fields of a gather / probability launch numbered by a selection, empty without one: ``sel`` (device
    int64 window numbers) and ``count`` (device int64 scalar, how many of them are valid) come together, with a
    ``cursor`` (device int64 scalar) and without ``idx``.  ``live``: the selection of a growing recording
    (:func:`live_select`), whose cursor is its own (:func:`live_gate_state`) and comes only with it."""
    if sel is None and count is None and not (live and cursor is not None):
        return {}
    if sel is None or count is None or idx is not None or cursor is None:
        raise ValueError("a selection is sel and count together, with a cursor and without idx")
    for t in (sel, count, cursor):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("sel / count / cursor must be contiguous int64 tensors on the device")
    if sel.dim() != 1 or count.numel() != 1 or cursor.numel() != 1:
        raise ValueError("sel must be a vector, count and cursor one number each")
    return {"sel": ptr(sel), "count": ptr(count), "cap": sel.numel(), "cursor": ptr(cursor)}


def gather_windows(rec: torch.Tensor, fs, ts, window: Tuple[int, int], B: int, idx: Optional[torch.Tensor] = None,
                   cursor: Optional[torch.Tensor] = None, lo: int = 0, hi: Optional[int] = None, taps: int = 0,
                   off: int = 0, lab_w: int = 2, sel: Optional[torch.Tensor] = None,
                   count: Optional[torch.Tensor] = None):
    """Windows of an HBM-resident recording ``rec`` [C, F, T] (fp32) -> (bf16 NHWC batch with C padded to 8, zero
    labels), the layout of :func:`gather_batch` of the materialised windows.  Window ``n = a * len(ts) + b`` starts
    at ``(fs[a], ts[b])``; batch row ``r`` holds window ``idx[r]`` (int64 [B]) or ``lo + cursor * B + r`` (``cursor``:
    a device int64 scalar).  Rows whose window number is outside ``[lo, hi)`` are zeros.  ``taps`` / ``off``: the
    1-channel stem's vertical tap packing, padded at the window's edges.

    ``sel`` / ``count`` (with ``cursor``; :func:`select_windows`): batch row ``r`` holds window
    ``sel[cursor * B + r]`` while ``cursor * B + r < count``, and is zeros beyond."""
    _check(rec, torch.float32)
    if rec.dim() != 3:
        raise ValueError("recording must be [C, F, T]")
    if (idx is None) == (cursor is None):
        raise ValueError("exactly one of idx / cursor")
    C, Fn, Tn = rec.shape
    fs, ts = _starts(fs, rec.device), _starts(ts, rec.device)
    for t in (idx, cursor):
        if t is not None:
            _check(t, torch.int64)
    if idx is not None and idx.numel() != B:
        raise ValueError("idx must hold B window numbers")
    hi = fs.numel() * ts.numel() if hi is None else hi
    d, out, lab = _gather_out(rec.device, fs, window, B, taps, off, lab_w)
    d.update({"rec": ptr(rec), "ts": ptr(ts), "C": C, "F": Fn, "T": Tn, "nt": ts.numel(), "idx": ptr(idx),
              "cursor": ptr(cursor), "lo": lo, "hi": hi})
    d.update(selection_args(sel, count, idx, cursor))
    lib().gather_windows(stream(), d)
    return out, lab


def window_probs(src: torch.Tensor, probs: torch.Tensor, idx: Optional[torch.Tensor] = None,
                 cursor: Optional[torch.Tensor] = None, lo: int = 0, hi: Optional[int] = None,
                 ncls: Optional[Sequence[int]] = None, sel: Optional[torch.Tensor] = None,
                 count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The batch's class probabilities into the resident table ``probs`` [N, K] (fp32, in place): row ``r`` of the
    batch goes to row ``idx[r]`` / ``lo + cursor * B + r``; rows outside ``[lo, hi)`` are skipped.  ``ncls`` given
    (Models A/B): ``src`` is the heads' log-probabilities [T, B, 16] and the table holds ``exp`` of the first
    ``ncls[t]`` columns of every task side by side.  Otherwise (Model C) ``src`` is logits [B, K] and the table holds
    their softmax.  In cursor form the launch advances the cursor by one.

    ``sel`` / ``count`` (with ``cursor``): row ``r`` goes to row ``sel[cursor * B + r]`` while ``cursor * B + r <
    count``; the rows beyond are skipped."""
    _check(probs, torch.float32)
    if (idx is None) == (cursor is None):
        raise ValueError("exactly one of idx / cursor")
    for t in (idx, cursor):
        if t is not None:
            _check(t, torch.int64)
    N, K = probs.shape
    B, d = _prob_source(src, K, ncls)
    if idx is not None and idx.numel() != B:
        raise ValueError("idx must hold B window numbers")
    d.update({"idx": ptr(idx), "cursor": ptr(cursor), "lo": lo, "hi": N if hi is None else hi, "probs": ptr(probs),
              "nprobs": N})
    d.update(selection_args(sel, count, idx, cursor))
    lib().window_probs(stream(), d)
    return probs


def window_power(rec: torch.Tensor, fs, ts, window: Tuple[int, int]) -> torch.Tensor:
    """The power of every window of a resident recording ``rec`` [C, F, T] (fp32): fp32 [len(fs) * len(ts)],
    ``power[a * len(ts) + b]`` = the mean over the channels of the mean over the window at ``(fs[a], ts[b])`` of
    ``(x - the window's own mean in that channel)^2`` -- :func:`sample_power`'s definition applied to a window
    (inference.window_power_reference; two passes with fp64 accumulators, a fixed reduction order)."""
    _check(rec, torch.float32)
    if rec.dim() != 3:
        raise ValueError("recording must be [C, F, T]")
    C, Fn, Tn = rec.shape
    fs, ts = _starts(fs, rec.device), _starts(ts, rec.device)
    power = torch.empty(fs.numel() * ts.numel(), device=rec.device, dtype=torch.float32)
    lib().window_power(stream(), {"rec": ptr(rec), "fs": ptr(fs), "ts": ptr(ts), "power": ptr(power), "C": C,
                                  "F": Fn, "T": Tn, "nf": fs.numel(), "nt": ts.numel(), "Wf": window[0],
                                  "Wt": window[1]})
    return power


def gate_ratio(gate_db: float) -> float:
    """``10^(gate_db / 10)`` rounded to fp32 once on the host: the factor on the noise floor above which a window's
    power makes it active."""
    import numpy as np
    return float(np.float32(10.0 ** (float(gate_db) / 10.0)))


def select_windows(power: torch.Tensor, floor: torch.Tensor, gate_db: float, nt: int, lo: int = 0,
                   hi: Optional[int] = None, sel: Optional[torch.Tensor] = None,
                   count: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None):
    """The active windows of ``[lo, hi)``: window ``n`` is active iff ``not (power[n] < floor[n // nt] * ratio)`` with
    ``ratio`` = :func:`gate_ratio` and one fp32 multiply, so a NaN power is active.  ``power``: fp32 [N] on the
    device; ``floor``: fp32, one noise floor per fiber start.  Returns ``(sel, count, active)``: ``sel`` int64 (at
    least ``hi - lo`` entries) whose first ``count`` entries are the active window numbers in ascending order -- the
    rest is left as it was, -1 in a buffer allocated here; ``count`` a device int64 scalar; ``active`` uint8 [N],
    zero outside ``[lo, hi)``.  Buffers passed in are written in place.  The order is that of the window numbers on
    every run (block counts, a scan, a ranked scatter; no atomics)."""
    _check(power, torch.float32)
    _check(floor, torch.float32)
    N = power.numel()
    hi = N if hi is None else hi
    dev = power.device
    if sel is None:
        sel = torch.full((max(hi - lo, 1),), -1, dtype=torch.int64, device=dev)
    if count is None:
        count = torch.zeros(1, dtype=torch.int64, device=dev)
    if active is None:
        active = torch.empty(N, dtype=torch.uint8, device=dev)
    _check(sel, torch.int64)
    _check(count, torch.int64)
    _check(active, torch.uint8)
    if active.numel() != N or count.numel() != 1:
        raise ValueError("active must hold one flag per window and count one number")
    offs = torch.empty(lib().select_blocks(N), dtype=torch.int64, device=dev)
    lib().select_windows(stream(), {"power": ptr(power), "floor": ptr(floor), "ratio": gate_ratio(gate_db), "N": N,
                                    "lo": int(lo), "hi": int(hi), "nfloor": floor.numel(), "nt": int(nt),
                                    "active": ptr(active), "sel": ptr(sel), "cap": sel.numel(), "offs": ptr(offs),
                                    "noffs": offs.numel(), "count": ptr(count)})
    return sel, count, active


def window_cell_weights(starts, win: int, length: int, cell: int):
    """fp64 [windows, cells]: the weight of window ``a`` in cell ``i`` of one axis, when a sample's value is the
    mean of the windows covering it and a cell's value the mean of its samples -- the sum over the samples the
    window shares with the cell of 1 / (windows covering the sample), over the cell's size.  A cell's weights sum
    to 1.  Raises if a sample of ``[0, length)`` is in no window."""
    import numpy as np
    s = np.asarray(starts, dtype=np.int64)
    if s.ndim != 1 or len(s) < 1 or (s < 0).any() or (s + win > length).any():
        raise ValueError("window starts outside the recording")
    cover = np.zeros(length + 1)
    np.add.at(cover, s, 1)
    np.add.at(cover, s + win, -1)
    cover = np.cumsum(cover)[:length]
    if (cover <= 0).any():
        raise ValueError("the window starts do not cover the recording")
    ncell = -(-length // cell)
    csum = np.concatenate([[0.0], np.cumsum(1.0 / cover)])  # csum[x] = sum of 1 / cover over [0, x)
    c0 = np.arange(ncell, dtype=np.int64) * cell
    c1 = np.minimum(c0 + cell, length)
    lo = np.maximum(s[:, None], c0[None])
    hi = np.maximum(np.minimum(s[:, None] + win, c1[None]), lo)
    return (csum[hi] - csum[lo]) / (c1 - c0)[None]


def _weight_band(w, starts, win: int, cell: int, device) -> torch.Tensor:
    """The nonzero band of :func:`window_cell_weights` as the kernel reads it: fp32 [windows, (win - 1) // cell + 2],
    window ``a``'s cells from ``starts[a] // cell`` on."""
    import numpy as np
    m = (win - 1) // cell + 2
    j = np.asarray(starts, dtype=np.int64)[:, None] // cell + np.arange(m)[None]
    band = np.where(j < w.shape[1], np.take_along_axis(w, np.minimum(j, w.shape[1] - 1), 1), 0.0)
    return torch.from_numpy(band.astype(np.float32)).to(device).contiguous()


def _axis_tables(starts, win: int, length: int, cell: int, device):
    """One axis of a map launch: the int32 device start table and the fp32 weight band of its windows."""
    w = window_cell_weights(starts, win, length, cell)
    return _starts(starts, device), _weight_band(w, starts, win, cell, device)


def window_map(probs: torch.Tensor, fs, ts, shape: Tuple[int, int], window: Tuple[int, int],
               cell: Tuple[int, int]) -> torch.Tensor:
    """Per-window probabilities [len(fs) * len(ts), K] -> cell map [K, ceil(F / cf), ceil(T / ct)] (fp32): a
    sample's value is the mean of the windows that cover it, a cell's value the mean of its samples.
    ``fs`` / ``ts``: host window-start tables that cover ``shape`` = (F, T) (inference.window_starts); the per-axis
    weights (:func:`window_cell_weights`) are computed on the host in fp64, the sums run on the device."""
    _check(probs, torch.float32)
    fs_h, ts_h = [int(v) for v in fs], [int(v) for v in ts]
    N, K = probs.shape
    if N != len(fs_h) * len(ts_h):
        raise ValueError("probs must have one row per window")
    nfc, ntc = -(-shape[0] // cell[0]), -(-shape[1] // cell[1])
    fs_d, wf = _axis_tables(fs_h, window[0], shape[0], cell[0], probs.device)
    ts_d, wt = _axis_tables(ts_h, window[1], shape[1], cell[1], probs.device)
    out = torch.empty(K, nfc, ntc, device=probs.device, dtype=torch.float32)
    lib().window_map(stream(), {"probs": ptr(probs), "fs": ptr(fs_d), "ts": ptr(ts_d), "map": ptr(out), "K": K,
                                "F": shape[0], "T": shape[1], "Wf": window[0], "Wt": window[1], "cf": cell[0],
                                "ct": cell[1], "nfc": nfc, "ntc": ntc, "wf": ptr(wf), "wt": ptr(wt),
                                "mf": wf.shape[1], "mt": wt.shape[1]}, fs_h, ts_h)
    return out


# ---- live inference on a growing recording (csrc/live.hip) -----------------------------------------------------
LIVE_TOTAL, LIVE_AVAIL, LIVE_NEXT, LIVE_JEND, LIVE_TEND, LIVE_NSTATE = range(6)


def live_state(device) -> torch.Tensor:
    """The device scalars of a live recording, int64 [LIVE_NSTATE]: total, avail, next = 0 and no end-aligned time
    index (jend = -1)."""
    s = torch.zeros(LIVE_NSTATE, dtype=torch.int64)
    s[LIVE_JEND] = -1
    return s.to(device)


def _live_scalars(state: torch.Tensor) -> int:
    _check(state, torch.int64)
    if state.numel() != LIVE_NSTATE:
        raise ValueError(f"state must hold {LIVE_NSTATE} int64 scalars (live_state)")
    return ptr(state)


def _live_args(ring: torch.Tensor, state: torch.Tensor, nf: int, st: int, Wt: int) -> dict:
    _check(ring, torch.float32)
    if ring.dim() != 3:
        raise ValueError("ring must be [C, F, R]")
    C, Fn, R = ring.shape
    if R < Wt + 1:
        raise ValueError(f"a ring of {R} time columns is below the window's {Wt} + 1")
    if st < 1 or nf < 1:
        raise ValueError("time stride and fiber window count must be positive")
    return {"ring": ptr(ring), "state": _live_scalars(state), "C": C, "F": Fn, "R": R, "nf": int(nf), "st": int(st),
            "Wt": int(Wt)}


def ring_append(ring: torch.Tensor, state: torch.Tensor, chunk: Optional[torch.Tensor], nf: int, st: int, Wt: int,
                flush: bool = False) -> None:
    """Append ``chunk`` [C, F, n] (fp32, ``n <= R - Wt``) to the time ring ``ring`` [C, F, R] -- sample ``t`` at
    column ``t mod R`` -- and advance the device scalars ``state`` (:func:`live_state`): ``total += n`` and ``avail``,
    the number of window numbers ``j * nf + a`` with ``j * st + Wt <= total``.  ``flush``: the stream ends at the new
    total (``chunk`` may be None): if ``(total - Wt) mod st != 0`` the end-aligned time index becomes available."""
    d = _live_args(ring, state, nf, st, Wt)
    n = 0
    if chunk is not None:
        _check(chunk, torch.float32)
        if chunk.dim() != 3 or tuple(chunk.shape[:2]) != tuple(ring.shape[:2]):
            raise ValueError(f"chunk must be [{ring.shape[0]}, {ring.shape[1]}, n], got {tuple(chunk.shape)}")
        n = chunk.shape[2]
        if n > ring.shape[2] - Wt:
            raise ValueError(f"a chunk of {n} samples overwrites data of a window not yet evaluated: at most "
                             f"R - Wt = {ring.shape[2] - Wt}")
    if n == 0 and not flush:
        raise ValueError("an empty chunk")
    d.update({"chunk": ptr(chunk) if n else 0, "n": n, "flush": int(flush)})
    lib().ring_append(stream(), d)


def gather_windows_ring(ring: torch.Tensor, state: torch.Tensor, fs, st: int, window: Tuple[int, int], B: int,
                        taps: int = 0, off: int = 0, lab_w: int = 2, sel: Optional[torch.Tensor] = None,
                        count: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None):
    """:func:`gather_windows` from the time ring: batch row ``r`` holds window ``next + r`` = ``(j, a)``, fiber start
    ``fs[a]``, time start ``j * st`` (``tend`` for the end-aligned index), columns taken ``mod R``; rows from
    ``avail`` on are zeros.  Returns (bf16 NHWC-8 batch, zero labels).

    ``sel`` / ``count`` / ``cursor`` (together; :func:`live_select`, :func:`live_gate_state`): row ``r`` holds window
    ``sel[cursor * B + r]`` while that entry is below ``count``, zeros beyond."""
    fs = _starts(fs, ring.device)
    d = _live_args(ring, state, fs.numel(), st, window[1])
    g, out, lab = _gather_out(ring.device, fs, window, B, taps, off, lab_w)
    d.update(g)
    d.update(selection_args(sel, count, None, cursor, live=True))
    lib().gather_windows_ring(stream(), d)
    return out, lab


def live_probs(src: torch.Tensor, table: torch.Tensor, state: torch.Tensor, nf: int, jcap: int,
               ncls: Optional[Sequence[int]] = None, sel: Optional[torch.Tensor] = None,
               count: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`window_probs` for the live numbering: batch row ``r`` is window ``next + r`` = ``(j, a)`` and goes to
    row ``(j mod jcap) * nf + a`` of the ring table ``table`` [>= jcap * nf, K] (in place); rows from ``avail`` on are
    skipped.  The launch then advances ``next`` by the number of valid rows.

    ``sel`` / ``count`` / ``cursor`` (together): batch row ``r`` is window ``sel[cursor * B + r]`` while that entry
    is below the count, and the table is the gated one, [>= jcap * nf, K + 1] -- columns ``0 .. K - 1`` the
    probabilities, column ``K`` 1.0, "evaluated".  The launch then advances the cursor by one."""
    _check(table, torch.float32)
    s = selection_args(sel, count, None, cursor, live=True)
    N, pitch = table.shape
    if jcap < 1 or nf < 1 or N < jcap * nf:
        raise ValueError(f"a table of {N} rows is below jcap * nf = {jcap * nf}")
    _, d = _prob_source(src, pitch - int(bool(s)), ncls)
    d.update(s)
    d.update({"state": _live_scalars(state), "nf": int(nf), "table": ptr(table), "nrows": N, "pitch": pitch,
              "Jcap": int(jcap)})
    lib().live_probs(stream(), d)
    return table


# ---- the activity gate of a growing recording (csrc/live_gate.hip) ----------------------------------------------
# Three rings of jcap time indices -- the windows' powers, their noise floors and their flags -- at row
# (j mod jcap) * nf + a like the ring table, and a selection (sel, count, cursor) that gather_windows_ring and
# live_probs take to number the captured step's rows.  Every launch works on the new window numbers [n0, n1): whole
# time indices, at most jcap of them.
MAX_FLOOR_HISTORY = 1024  # running_floor keeps a column's trailing powers in LDS


def live_gate_state(device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The device scalars of a live selection, ``(cursor, count)``: two int64 [1] views of one small tensor of their
    own (:func:`live_state` keeps its LIVE_NSTATE scalars), both 0."""
    s = torch.zeros(2, dtype=torch.int64, device=device)
    return s[0:1], s[1:2]


def _gate_rings(nf: int, jcap: int, n0: int, n1: int, **rings) -> dict:
    """The range and the rings of a live gate launch, checked: ``rings`` by launch field name, each a contiguous
    device vector of ``jcap * nf`` entries (``active``: uint8, the others fp32)."""
    nf, jcap, n0, n1 = int(nf), int(jcap), int(n0), int(n1)
    if nf < 1 or jcap < 1 or not 0 <= n0 <= n1 or n0 % nf or n1 % nf or (n1 - n0) // nf > jcap:
        raise ValueError(f"windows [{n0}, {n1}) must be whole time indices of {nf} windows, at most jcap = {jcap}")
    d = {"nf": nf, "Jcap": jcap, "n0": n0, "n1": n1}
    for k, t in rings.items():
        _check(t, torch.uint8 if k == "active" else torch.float32)
        if t.dim() != 1 or t.numel() != jcap * nf:
            raise ValueError(f"the {k} ring must hold jcap * nf = {jcap * nf} entries")
        d[k] = ptr(t)
    return d


def ring_window_power(ring: torch.Tensor, state: torch.Tensor, fs, st: int, window: Tuple[int, int],
                      power: torch.Tensor, jcap: int, n0: int, n1: int) -> torch.Tensor:
    """:func:`window_power` of the live windows ``[n0, n1)`` (``n = j * nf + a``, start ``(fs[a], j * st)``, ``tend``
    for the end-aligned index) read from the time ring, into rows ``(j mod jcap) * nf + a`` of the power ring
    ``power`` (fp32 [jcap * nf], in place).  The accumulation is :func:`window_power`'s, so the powers have the bits
    of the linear recording's.  A window that is not available, or no longer in the ring, gets NaN."""
    fs = _starts(fs, ring.device)
    d = _live_args(ring, state, fs.numel(), st, window[1])
    d.update(_gate_rings(fs.numel(), jcap, n0, n1, power=power))
    d.update({"fs": ptr(fs), "Wf": window[0]})
    lib().ring_window_power(stream(), d)
    return power


def running_floor(power: torch.Tensor, floor: torch.Tensor, nf: int, jcap: int, n0: int, n1: int, history: int,
                  warmup: int) -> torch.Tensor:
    """The causal noise floor of the live windows ``[n0, n1)`` into the floor ring (in place): for window ``(j, a)``
    the lower median of the powers of fiber start ``a`` at the time indices ``max(0, j - history + 1) .. j`` (``m`` of
    them, row ``j`` included), NaN ordered last; 0 while ``m < warmup`` (inference.running_floor_reference).  A
    selection, so exact.  The power ring must still hold those indices: ``jcap >= history - 1 + (n1 - n0) / nf``."""
    d = _gate_rings(nf, jcap, n0, n1, power=power, floor=floor)
    if not 1 <= warmup <= history <= MAX_FLOOR_HISTORY:
        raise ValueError(f"1 <= warmup <= history <= {MAX_FLOOR_HISTORY}, got warmup {warmup}, history {history}")
    if jcap < history - 1 + (n1 - n0) // nf:
        raise ValueError(f"rings of {jcap} time indices are below history - 1 + the range's {(n1 - n0) // nf}")
    d.update({"history": int(history), "warmup": int(warmup)})
    lib().running_floor(stream(), d)
    return floor


def live_select(power: torch.Tensor, floor: torch.Tensor, active: torch.Tensor, table: torch.Tensor,
                state: torch.Tensor, sel: torch.Tensor, count: torch.Tensor, cursor: torch.Tensor, gate_db: float,
                nf: int, jcap: int, n0: int, n1: int) -> None:
    """The flags of the live windows ``[n0, n1)`` -- active iff ``not (power < floor * ratio)``, as
    :func:`select_windows` -- into the active ring; ``sel[:count]`` becomes the active window numbers in ascending
    order, the rest of ``sel`` is left as it was (``count`` / ``cursor``: :func:`live_gate_state`).  Every row of the range in the ring
    table ``table`` [>= jcap * nf, K + 1] is zeroed (the rows are recycled).  The last launch sets the batch
    cursor to 0 and ``state[LIVE_NEXT]`` to ``n1``."""
    _check(table, torch.float32)
    d = _gate_rings(nf, jcap, n0, n1, power=power, floor=floor, active=active)
    d.update(selection_args(sel, count, None, cursor, live=True))
    d["state"] = _live_scalars(state)
    if table.dim() != 2 or table.shape[0] < jcap * nf:
        raise ValueError(f"a table of {tuple(table.shape)} is below jcap * nf = {jcap * nf} rows")
    if sel.numel() < n1 - n0:
        raise ValueError(f"sel holds {sel.numel()} entries, the range {n1 - n0} windows")
    offs = torch.empty(max(1, lib().select_blocks(n1 - n0)), dtype=torch.int64, device=power.device)
    d.update({"ratio": gate_ratio(gate_db), "table": ptr(table), "nrows": table.shape[0], "pitch": table.shape[1],
              "offs": ptr(offs), "noffs": offs.numel()})
    lib().live_select(stream(), d)


def live_map(table: torch.Tensor, fs, F: int, Wf: int, cf: int, jcap: int, jlo, wt) -> torch.Tensor:
    """Cell columns of the map from the ring table ``table`` [>= jcap * len(fs), K] -> [K, ceil(F / cf), ncol]
    (fp32).  Column ``q`` of the call is ``sum_a sum_j wf[a, i] wt[q][j] table[(j mod jcap) * nf + a]`` over the time
    indices ``jlo[q] .. jlo[q] + len(wt[q]) - 1``: ``wt`` is a list of per-column fp64 weight vectors (the host's,
    inference.live_time_weights), rounded to fp32 here; the fiber weights are :func:`window_map`'s bands."""
    import numpy as np
    _check(table, torch.float32)
    fs_h = [int(v) for v in fs]
    N, K = table.shape
    ncol = len(jlo)
    if ncol < 1 or len(wt) != ncol:
        raise ValueError("one weight vector and one first time index per column")
    jn = [len(w) for w in wt]
    if min(jn) < 1 or max(jn) > jcap:
        raise ValueError(f"a column needs 1 .. jcap = {jcap} time indices, got {min(jn)} .. {max(jn)}")
    if N < jcap * len(fs_h):
        raise ValueError(f"a table of {N} rows is below jcap * nf = {jcap * len(fs_h)}")
    mw = max(jn)
    band = np.zeros((ncol, mw), dtype=np.float32)
    for q, w in enumerate(wt):
        band[q, :len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32)
    dev = table.device
    fs_d, wf = _axis_tables(fs_h, Wf, F, cf, dev)
    wt_d = torch.from_numpy(band).to(dev)
    jlo_d = torch.as_tensor([int(v) for v in jlo], dtype=torch.int64).to(dev)
    jn_d = torch.as_tensor(jn, dtype=torch.int32).to(dev)
    nfc = -(-F // cf)
    out = torch.empty(K, nfc, ncol, device=dev, dtype=torch.float32)
    lib().live_map(stream(), {"table": ptr(table), "fs": ptr(fs_d), "map": ptr(out), "wf": ptr(wf), "wt": ptr(wt_d),
                              "jlo": ptr(jlo_d), "jn": ptr(jn_d), "mf": wf.shape[1], "mw": mw, "K": K, "F": F,
                              "Wf": Wf, "cf": cf, "nfc": nfc, "Jcap": int(jcap), "nrows": N},
                   fs_h, [int(v) for v in jlo], jn)
    return out


# ---- raw-rate recordings: FIR and decimation ahead of the ring (csrc/resample.hip) ------------------------------
DECIMATE_TILE = 128  # outputs of one block (csrc/kernels.h)


def decimate_carry(rows: int, L: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two carry buffers of a decimated stream, fp32 [rows, L - 1] each: a launch reads one and writes the
    other, and the host flips them."""
    return (torch.zeros(rows, L - 1, device=device), torch.zeros(rows, L - 1, device=device))


def fir_decimate(raw: torch.Tensor, carry_in: Optional[torch.Tensor], carry_len: int, skip: int, taps: torch.Tensor,
                 D: int, out: Optional[torch.Tensor] = None, m: Optional[int] = None,
                 carry_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """One piece of a raw stream through the FIR ``taps`` (fp32 [L]) and decimation by ``D``
    (data/resample.py ``fir_decimate_reference`` is the definition).  ``raw``: [C, F, n] fp32 or int16, time
    contiguous (a slice along time of a contiguous tensor will do).  The piece's samples are the first
    ``carry_len`` columns of ``carry_in`` (fp32 [C * F, L - 1]; None: nothing carried) followed by ``raw[.., skip:]``;
    ``out`` (fp32 [C, F, m], the layout :func:`ring_append` takes) gets the ``m`` outputs they complete and
    ``carry_out`` (not ``carry_in``) the new tail, in its first columns -- ``DecimatorBook`` says how many.  Every
    output is one fp32 fma chain over the taps in a fixed order, so a stream has the same bits however it is cut.
    ``m``: checked against the count the other arguments imply (None: that count).  Returns ``(out, carry_out)``."""
    if raw.dim() != 3:
        raise ValueError(f"raw must be [C, F, n], got {tuple(raw.shape)}")
    if not raw.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if raw.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"raw must be float32 or int16, got {raw.dtype}")
    _check(taps, torch.float32)
    C, Fn, n = raw.shape
    rows, L, D = C * Fn, taps.numel(), int(D)
    if taps.dim() != 1 or not 1 <= L <= lib().DECIMATE_MAX_TAPS or not 1 <= D <= lib().DECIMATE_MAX_FACTOR:
        raise ValueError(f"1 <= D <= {lib().DECIMATE_MAX_FACTOR} and 1 <= L <= {lib().DECIMATE_MAX_TAPS} taps, got "
                         f"D = {D}, taps {tuple(taps.shape)}")
    if rows < 1:
        raise ValueError("raw has no rows")
    pitch = n
    if n > 0:
        pitch = raw.stride(1) if Fn > 1 else (raw.stride(0) if C > 1 else n)
        if raw.stride(2) != 1 or pitch < n or (C > 1 and raw.stride(0) != Fn * pitch):
            raise ValueError("raw must be contiguous along time with one row pitch")
    carry_len, skip = int(carry_len), int(skip)
    if not 0 <= carry_len <= L - 1 or skip < 0 or (skip > 0 and carry_len > 0):
        raise ValueError(f"0 <= carry_len <= L - 1 = {L - 1} and skip >= 0 (and nothing carried), got carry_len "
                         f"{carry_len}, skip {skip}")
    want = lib().fir_output_count(carry_len, skip, n, L, D)
    if m is None:
        m = want
    if int(m) != want:
        raise ValueError(f"a piece of {n} samples after a carry of {carry_len} and a skip of {skip} yields {want} "
                         f"outputs, not {m}")
    m = int(m)
    for name, c in (("carry_in", carry_in), ("carry_out", carry_out)):
        if c is not None:
            _check(c, torch.float32)
            if tuple(c.shape) != (rows, L - 1):
                raise ValueError(f"{name} must be [{rows}, {L - 1}], got {tuple(c.shape)}")
    if carry_len > 0 and carry_in is None:
        raise ValueError("carry_len > 0 without carry_in")
    if carry_out is None:
        carry_out = torch.zeros(rows, L - 1, device=raw.device)
    if carry_in is not None and L > 1 and carry_in.data_ptr() == carry_out.data_ptr():
        raise ValueError("carry_out must not be carry_in: a block reads the one while another writes the other")
    if out is None:
        out = torch.empty(C, Fn, m, device=raw.device)
    _check(out, torch.float32)
    if tuple(out.shape) != (C, Fn, m):
        raise ValueError(f"out must be [{C}, {Fn}, {m}], got {tuple(out.shape)}")
    lib().fir_decimate(stream(), {"raw": ptr(raw) if n else 0, "carry_in": ptr(carry_in) if carry_in is not None else 0,
                                  "taps": ptr(taps), "out": ptr(out) if m else 0, "carry_out": ptr(carry_out),
                                  "rows": rows, "n": n, "pitch": pitch, "m": m, "carry_len": carry_len, "skip": skip,
                                  "D": D, "L": L, "itype": 1 if raw.dtype == torch.int16 else 0})
    return out, carry_out


# ---- common-mode removal ahead of the windows (csrc/common_mode.hip) -------------------------------------------
def _time_rows(t: torch.Tensor, name: str) -> int:
    """The row pitch of ``t`` [C, F, n] as the kernels read it: fp32 on the device, contiguous along time with one
    pitch over all C * F rows (a slice along time of a contiguous tensor will do)."""
    if t.dim() != 3:
        raise ValueError(f"{name} must be [C, F, n], got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError("HIP ops need a GPU tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    C, Fn, n = t.shape
    if n == 0:
        return 0
    pitch = t.stride(1) if Fn > 1 else (t.stride(0) // Fn if C > 1 else n)
    if t.stride(2) != 1 or pitch < n or (C > 1 and t.stride(0) != Fn * pitch):
        raise ValueError(f"{name} must be contiguous along time with one row pitch")
    return pitch


def _span(t: torch.Tensor, count: int) -> Tuple[int, int]:
    return t.data_ptr(), t.data_ptr() + 4 * count


def common_mode(x: torch.Tensor, how: str, out: Optional[torch.Tensor] = None,
                trace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x`` [C, F, n] fp32 minus its common mode, the per-sample lower median (``how = "median"``) or mean
    (``"mean"``) over the fiber (data/common_mode.py ``common_mode_reference`` is the definition; the device gives
    its bits).  ``x`` and ``out`` are contiguous along time with one row pitch each; ``out`` (None: a new tensor) may
    be ``x`` itself -- a block owns whole columns -- but must not overlap it otherwise.  ``trace`` (None: a new
    tensor): contiguous fp32 [C, n], receives the value subtracted.  Returns ``(out, trace)``."""
    from ..data.common_mode import HOWS, as_common_mode
    how = as_common_mode(how)
    if how is None:
        raise ValueError("common_mode needs 'median' or 'mean'")
    pitch = _time_rows(x, "x")
    C, Fn, n = x.shape
    if C < 1 or not 1 <= Fn <= lib().COMMON_MODE_MAX_F:
        raise ValueError(f"x needs C >= 1 and 1 <= F <= {lib().COMMON_MODE_MAX_F}, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(C, Fn, n, device=x.device)
    out_pitch = _time_rows(out, "out")
    if tuple(out.shape) != (C, Fn, n):
        raise ValueError(f"out must be [{C}, {Fn}, {n}], got {tuple(out.shape)}")
    if trace is None:
        trace = torch.empty(C, n, device=x.device)
    _check(trace, torch.float32)
    if tuple(trace.shape) != (C, n):
        raise ValueError(f"trace must be [{C}, {n}], got {tuple(trace.shape)}")
    tiles = (n + lib().COMMON_MODE_TILE - 1) // lib().COMMON_MODE_TILE
    if n >= 1 << 31 or C * tiles >= 1 << 31 or C * Fn >= 1 << 32 or max(pitch, out_pitch) >= 1 << 31:
        raise ValueError(f"x {tuple(x.shape)} is beyond what one launch addresses")
    if n == 0:
        return out, trace

    def overlap(p, q):
        return p[0] < q[1] and q[0] < p[1]
    xs, os_ = _span(x, (C * Fn - 1) * pitch + n), _span(out, (C * Fn - 1) * out_pitch + n)
    if (out_pitch != pitch) if out.data_ptr() == x.data_ptr() else overlap(xs, os_):
        raise ValueError("out must be x itself or apart from it: a block reads what another writes otherwise")
    ts_ = _span(trace, C * n)
    if overlap(ts_, xs) or overlap(ts_, os_):
        raise ValueError("trace must not overlap x or out")
    lib().common_mode(stream(), {"x": ptr(x), "out": ptr(out), "trace": ptr(trace), "rows": C, "F": Fn, "n": n,
                                 "pitch": pitch, "out_pitch": out_pitch, "how": HOWS.index(how)})
    return out, trace
