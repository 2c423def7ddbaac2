"""The fused backward join at kernel level against the fp64 reference of tests/bwd_ref.py (itself checked against
fp64 autograd in tests/test_bwd_ref.py).

A. The data-gradient epilogue of every conv kernel family (csrc/conv.hip conv_igemm at both pipeline depths,
   csrc/conv_lds.hip LDS / LDS-DMA in both rings / patch / persistent patch, split K included): added gradient
   sources (ConvArgs::add), fused BN-backward sums of the tail the gradient feeds (ConvArgs::bpart; ACT_RELU and
   ADD_RELU with an identity or a projection shortcut), groups, a tail narrower than the gradient, a tail shared
   by the groups, fewer replicas -- and the apply-only tail (fused = 2) that consumes those sums.
B. The BN tail backward of csrc/bn.hip: several gradient sources with mixed pitches, the stored-dz form, the
   reduce-only + apply-only composition with ``gscale`` (SyncBN), groups, the single-launch kernel at its three
   register depths, ceil-mode pooling windows.

Bounds (none derived from what the kernels give):
  dx            |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| per element: one bf16 ulp (half an ulp of rounding plus an
                fp32 accumulation that may straddle a rounding boundary).
  statistics    per channel, against fp64 sums over the kernel's OWN stored dx and the fp64 mask:
                |got_c - ref_c| <= 1e-4 sum|terms_c| + sum over the mask-ambiguous elements of |term|.  1e-4 covers
                the worst-case sequential fp32 accumulation of the 1428 addends (1428 * 2^-24 = 8.5e-5); the
                single-launch tail at 4096 pixels sums in a tree of depth 4 + 6 + 16, far below that.  One missing
                element is 7e-4 of sum|terms_c|.
  activations   relative L2 6e-3, d(gamma) / d(beta) of the apply-only tail relative L2 1e-5 (the layer-local
                bounds of tests/test_mtl_layer_local_gpu.py TOL); the join inputs have no ReLU argument within
                bwd_ref.JOIN_MARGIN of zero, so no mask of theirs can flip.

Worst observed values on MI355X (printed by every test, ``Checker.done``):
  A  dx err / bound 0.992 (an fp32 sum straddling a rounding boundary: one ulp = 2^-8 |ref| at most, by construction
     below the bound); sums err / sum|terms| 1.7e-8 (bound 1e-4); apply-only tail: dy 1.67e-3, dy2 1.67e-3 (6e-3),
     side 0 (dz is the stored bf16 dx under the mask, exactly), d(gamma) 1.4e-7, d(beta) 2.7e-8 (1e-5).
  B  sums err / sum|terms| 3.0e-8 (bound 1e-4); dy 2.5e-3, dy2 2.5e-3, side 1.8e-3 (6e-3; the larger values are
     the stored-dz form, whose dz carries a bf16 rounding).
  Every family ran the configs its minimum names; no kernel or binding had to change.
"""
import math

import pytest
import torch

import bwd_ref as R

pytestmark = pytest.mark.gpu

NREP = 32
B, H, W = R.BASE
C = 32
TOL_ACT, TOL_PAR = 6e-3, 1e-5


@pytest.fixture(scope="module")
def fn():
    from mtl_das_pytorch_amd.ops import functional as fn
    return fn


class Checker:
    """Collects every violated bound and the worst observed value of each kind of assertion."""

    def __init__(self):
        self.worst, self.bad = {}, []

    def _note(self, kind, v):
        self.worst[kind] = max(self.worst.get(kind, 0.0), v)

    def elementwise(self, what, got, ref):
        """dx against the fp64 join: one bf16 ulp."""
        ref = ref.to(got.device)
        err = (got.double() - ref).abs()
        bound = ref.abs() * 2.0 ** -8 + 1e-5 * ref.abs().max()
        v = (err / bound).max().item()
        self._note("dx err / bound", v)
        if not v <= 1.0:
            self.bad.append((what, "dx", f"{v:.3g} x bound, {int((err > bound).sum())} elements"))

    def sums(self, what, got, terms, ambt):
        """Per-channel sums: ``got`` [C] against ``terms`` [..., C] (fp64), ``ambt`` the |term| of the ambiguous
        elements."""
        red = tuple(range(terms.dim() - 1))
        ref, mag = terms.sum(red), terms.abs().sum(red)
        bound = 1e-4 * mag + (ambt.sum(red) if ambt is not None else 0.0)
        err = (got.double() - ref).abs()
        self._note("sums err / sum|terms|", (err / mag.clamp_min(1e-300)).max().item())
        if not bool((err <= bound).all()):
            c = int((err / bound.clamp_min(1e-300)).argmax())
            self.bad.append((what, "sums", f"channel {c}: err {err[c].item():.3e} bound {bound[c].item():.3e}"))

    def l2(self, kind, what, got, ref, tol):
        ref = ref.to(got.device)
        if not bool(torch.isfinite(got.float()).all()):
            self.bad.append((what, kind, "not written (non-finite)"))
            return
        v = ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
        self._note(kind + " rel L2", v)
        if not v < tol:
            self.bad.append((what, kind, f"{v:.3e}"))

    def true(self, what, cond):
        if not cond:
            self.bad.append((what, "condition"))

    def done(self):
        print("worst observed", {k: f"{v:.2e}" for k, v in self.worst.items()})
        assert not self.bad, self.bad[:20]


# ---------------------------------------------------------------------------------------------------
# inputs
class Tail:
    """Device copies of bwd_ref.tail_inputs and, per kind, the fp64 mask, ambiguity map and xhat (on the device)."""

    def __init__(self, seed, shape, Cc):
        self.t = R.tail_inputs(seed, *shape, Cc)
        self.dev = {k: v.cuda() for k, v in self.t.items()}
        self.n = shape[0] * shape[1] * shape[2]
        k, k2 = self.t["k"].double(), self.t["k2"].double()
        self.xh = ((self.t["y"].double() - k[2]) * k[3]).cuda()
        self.xh2 = ((self.t["y2"].double() - k2[2]) * k2[3]).cuda()
        self._m, self._bn = {}, {}

    def mask(self, name):
        if name not in self._m:
            m, amb = R.kind_mask(name, self.t)
            self._m[name] = (m.cuda(), amb.double().cuda() if amb is not None else None)
        return self._m[name]

    def r(self, name):
        kind, proj = R.KINDS[name]
        return self.dev["y2"] if proj else (self.dev["r"] if kind in (R.SIGMUL, R.ADD_RELU) else None)


def bn_of(fn, tails, which="", pnrep=None):
    """Kernel BN descriptor of the BN of y (``which`` = "") or of y2 ("2": the projection shortcut's BN) of one Tail,
    or of a list of Tails as groups.  The constants are the reference's (bwd_ref.batch_consts)."""
    grouped = isinstance(tails, (list, tuple))
    if not grouped and pnrep is None:
        if which not in tails._bn:
            tails._bn[which] = _bn_of(fn, [tails], which, None, False)
        return tails._bn[which]
    return _bn_of(fn, list(tails) if grouped else [tails], which, pnrep, grouped)


def _bn_of(fn, ts, which, pnrep, grouped):
    ys = [t.t["y2" if which else "y"].double() for t in ts]
    Cc = ys[0].shape[-1]
    stats = torch.zeros(len(ts), NREP, 2, Cc, dtype=torch.float64)
    for z, y in enumerate(ys):
        stats[z, 0, 0], stats[z, 0, 1] = y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))
    par = [torch.stack([t.t[n + which] for t in ts]) for n in ("gamma", "beta")]
    par += [torch.zeros(len(ts), Cc), torch.ones(len(ts), Cc)]
    if not grouped:
        par = [p[0] for p in par]
    consts = torch.stack([t.t["k" + which] for t in ts]).contiguous().cuda()
    return fn.bn_args(stats.cuda(), *[p.contiguous().cuda() for p in par],
                      torch.zeros(len(ts), dtype=torch.int64, device="cuda"), count=ts[0].n, consts=consts, pnrep=pnrep)


def sliced(src, width, off):
    """``src`` as a column slice of a wider device buffer (pitch ``width``) whose other columns hold noise."""
    buf = torch.randn(tuple(src.shape[:-1]) + (width,), generator=torch.Generator().manual_seed(off)).bfloat16().cuda()
    buf[..., off:off + src.shape[-1]] = src.cuda()
    return buf[..., off:off + src.shape[-1]]


class Conv:
    """One conv's data-gradient inputs: bf16-rounded weights [Co, Ci, k, k], bf16 dy, ``nsrc`` bf16 sources (CPU);
    ``g(n)`` = the fp64 join with the first n sources, on the device."""

    def __init__(self, seed, Ci, Co, k, s, p, nsrc):
        gen = torch.Generator().manual_seed(seed)
        self.k, self.s, self.p, self.Ci, self.Co = k, s, p, Ci, Co
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.w = (torch.randn(Co, Ci, k, k, generator=gen) / math.sqrt(Co * k * k)).bfloat16().float()
        self.dy = torch.randn(B, Ho, Wo, Co, generator=gen).bfloat16()
        self.srcs = [torch.randn(B, H, W, Ci, generator=gen).bfloat16() for _ in range(nsrc)]
        # the first source is a column slice (pitch 64) of a wider buffer
        self.dsrcs = [sliced(t, 64, 8) if i == 0 else t.cuda() for i, t in enumerate(self.srcs)]
        self._g = {}

    def g(self, n):
        if n not in self._g:
            self._g[n] = R.join(self.w, self.dy, (H, W), self.s, self.p, self.srcs[:n]).cuda()
        return self._g[n]


@pytest.fixture(scope="module")
def tails():
    return [Tail(seed, R.BASE, C) for seed in R.JOIN_SEEDS]


# ---------------------------------------------------------------------------------------------------
# A. the dgrad epilogue of every kernel family
def _families(fn):
    return {
        "igemm": list(range(14)),
        "igemm_deep": [fn.CONV_DEEP_CFG0 + t for t in range(14)],
        "lds": [fn.lds_cfg(t, kc, sp) for t in range(8) for kc in (64, 128) if not (kc == 128 and t == 3)
                for sp in (1, 2)],
        "glds": [fn.glds_cfg(t, sp, deep) for deep in (False, True) for t in (fn.GDEEP_TILES if deep else range(8))
                 for sp in (1, 2)],
        "patch": [fn.patch_cfg(t, cb) for t in range(len(fn.PATCH_TILES)) for cb in fn.PATCH_CB],
        "patch_persistent": [fn.patch_cfg(t, cb, True) for t in range(len(fn.PATCH_TILES)) for cb in fn.PATCH_CB],
    }


FAMILIES = ["igemm", "igemm_deep", "lds", "glds", "patch", "patch_persistent"]
GEMM_FAMILIES = FAMILIES[:4]
# configs of each family that must accept the (3x3 / s1 / p1, dy channels Co) shape: all of the implicit-GEMM
# families; the patch kernels stage dy in slices of 16 / 32 / 64 channels (Co = 48: the five 16-channel configs),
# the persistent form holds one slice (Co == cb: none at 48, the five 32-channel configs at 32)
MIN_RAN = {"igemm": 14, "igemm_deep": 14, "lds": 30, "glds": 28}
MIN_RAN_PATCH = {("patch", 48): 5, ("patch", 32): 10, ("patch_persistent", 32): 5}


def _prepare(fn, *a, **kw):
    """The prepared launch, or None when the config does not take the shape."""
    try:
        return fn.prepare_conv2d_dgrad(*a, **kw)
    except ValueError:
        return None


def _tickets_zero(chk, what, call):
    if call._ws:
        chk.true(what + " split-K tickets", int(call._ws[1].abs().sum()) == 0)


def _check_part(chk, what, rows, dx, tail, name):
    """The three statistic rows [3, C'] against fp64 sums over the kernel's own stored ``dx`` [..., C']."""
    m, amb = tail.mask(name)
    g = dx.double()
    proj = R.KINDS[name][1]
    for row, f in enumerate((None, tail.xh, tail.xh2 if proj else None)):
        if row == 2 and not proj:
            chk.true(what + " row 2 untouched", bool((rows[2] == 0).all()))
            continue
        terms = g * m if f is None else g * m * f
        ambt = None if amb is None else (g.abs() * amb if f is None else (g * f).abs() * amb)
        chk.sums(f"{what} row {row}", rows[row], terms, ambt)


def _bnb(fn, tail, name, part, **kw):
    kind, proj = R.KINDS[name]
    d = {"y": tail.dev["y"], "bn": kw.pop("bn", None) or bn_of(fn, tail), "part": part, "kind": kind}
    if kind == R.ADD_RELU:
        d["r"] = tail.r(name)
    if proj:
        d["bn2"] = kw.pop("bn2", None) or bn_of(fn, tail, "2")
    d.update(kw)
    return d


def _apply_only(fn, chk, what, tail, name, dx, part):
    """The apply-only tail (fused = 2) on the epilogue's sums, against the reference tail of the stored dx."""
    kind, proj = R.KINDS[name]
    par = [torch.full((C,), float("nan"), device="cuda") for _ in range(4)]
    out = {k: torch.full((B, H, W, C), float("nan"), device="cuda", dtype=torch.bfloat16) for k in ("dy", "side", "dy2")}
    dy, side, dy2 = fn.bn_tail_backward(kind, tail.dev["y"], bn_of(fn, tail), [dx], par[0], par[1], r=tail.r(name),
                                        bn2=bn_of(fn, tail, "2") if proj else None, dgamma2=par[2], dbeta2=par[3],
                                        part=part, out=out)
    ref = R.kind_tail(name, tail.t, dx)
    chk.l2("apply dy", what, dy, ref["dy"], TOL_ACT)
    chk.l2("apply dgamma", what, par[0], ref["dgamma"], TOL_PAR)
    chk.l2("apply dbeta", what, par[1], ref["dbeta"], TOL_PAR)
    if proj:
        chk.l2("apply dy2", what, dy2, ref["dy2"], TOL_ACT)
        chk.l2("apply dgamma", what + " (2)", par[2], ref["dgamma2"], TOL_PAR)
        chk.l2("apply dbeta", what + " (2)", par[3], ref["dbeta2"], TOL_PAR)
    elif kind == R.ADD_RELU:
        chk.l2("apply side", what, side, ref["side"], TOL_ACT)  # written by the apply pass itself


@pytest.mark.parametrize("family,Co", [(f, 48) for f in FAMILIES[:5]] + [("patch", 32), ("patch_persistent", 32)])
def test_join_sources_and_residual_stats(fn, tails, family, Co):
    """Case 1: 3x3 / s1 / p1, Co -> 32 with 1, 2, 3 added sources (one a slice of pitch 64) feeding an ACT_RELU, an
    identity-shortcut and a projection-shortcut ADD_RELU tail; then the apply-only tail.  (Co = 32: the patch
    kernels' 32-channel slices, which the persistent form needs.)"""
    conv, tail, chk, ran = Conv(100, C, Co, 3, 1, 1, 3), tails[0], Checker(), 0
    dy = conv.dy.cuda()
    for cfg in _families(fn)[family]:
        part = torch.zeros(NREP, 3, C, device="cuda", dtype=torch.float64)
        if _prepare(fn, dy, conv.w.cuda(), (H, W), 1, 1, cfg=cfg, bn_stats=_bnb(fn, tail, "add_proj", part)) is None:
            continue
        ran += 1
        for nsrc in (1, 2, 3):
            for name in R.JOIN_KINDS:
                part = torch.zeros(NREP, 3, C, device="cuda", dtype=torch.float64)
                call = fn.prepare_conv2d_dgrad(dy, conv.w.cuda(), (H, W), 1, 1, cfg=cfg, add=conv.dsrcs[:nsrc],
                                               bn_stats=_bnb(fn, tail, name, part))
                dx = call.run()
                what = f"cfg {cfg} {nsrc} sources {name}"
                chk.elementwise(what, dx, conv.g(nsrc))
                _check_part(chk, what, part.sum(0), dx, tail, name)
                _tickets_zero(chk, what, call)
                _apply_only(fn, chk, what, tail, name, dx, part)
    chk.done()
    need = MIN_RAN[family] if family in MIN_RAN else MIN_RAN_PATCH[(family, Co)]
    assert ran >= need, (ran, need)


@pytest.mark.parametrize("k,p", [(3, 1), (1, 0)])
@pytest.mark.parametrize("family", GEMM_FAMILIES)
def test_join_strided(fn, tails, family, k, p):
    """Case 2: the stride-2 dgrads (3x3 / p1 and the 1x1 / p0 projection shortcut, three of whose four sub-pixel
    phases have no tap): every pixel still receives the 2 added sources and enters the ADD_RELU statistics."""
    conv, tail, chk, ran = Conv(200 + k, C, 48, k, 2, p, 2), tails[0], Checker(), 0
    for cfg in _families(fn)[family]:
        part = torch.zeros(NREP, 3, C, device="cuda", dtype=torch.float64)
        call = _prepare(fn, conv.dy.cuda(), conv.w.cuda(), (H, W), 2, p, cfg=cfg, add=conv.dsrcs,
                        bn_stats=_bnb(fn, tail, "add", part))
        if call is None:
            continue
        dx = call.run()
        ran += 1
        chk.elementwise(f"cfg {cfg}", dx, conv.g(2))
        _check_part(chk, f"cfg {cfg}", part.sum(0), dx, tail, "add")
        _tickets_zero(chk, f"cfg {cfg}", call)
    chk.done()
    assert ran >= MIN_RAN[family], ran


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_join_groups(fn, tails, family, shared):
    """Case 3: G = 2 with per-group weights, dy, sources, y, BN parameters and part (projection-shortcut tail);
    ``shared``: pgs = 0 -- one y / r / part, both groups add their share (identity-shortcut tail)."""
    Co = 32 if family == "patch_persistent" else 48
    convs, chk, ran = [Conv(300 + z, C, Co, 3, 1, 1, 1) for z in range(2)], Checker(), 0
    name = "add" if shared else "add_proj"
    dy, w = torch.stack([c.dy for c in convs]).cuda(), torch.stack([c.w for c in convs]).cuda()
    add = [torch.stack([c.srcs[0] for c in convs]).cuda()]
    for cfg in _families(fn)[family]:
        if shared:
            part = torch.zeros(NREP, 3, C, device="cuda", dtype=torch.float64)
            bnb = _bnb(fn, tails[0], name, part, pgs=0)
        else:
            part = torch.zeros(2, NREP, 3, C, device="cuda", dtype=torch.float64)
            bnb = _bnb(fn, tails[0], name, part, bn=bn_of(fn, tails), bn2=bn_of(fn, tails, "2"))
            bnb["y"], bnb["r"] = (torch.stack([t.dev[n] for t in tails]) for n in ("y", "y2"))
        call = _prepare(fn, dy, w, (H, W), 1, 1, cfg=cfg, add=add, bn_stats=bnb, groups=2)
        if call is None:
            continue
        dx = call.run()
        ran += 1
        for z in range(2):
            chk.elementwise(f"cfg {cfg} group {z}", dx[z], convs[z].g(1))
        if shared:  # the sums are linear in the gradient: both groups' dx under the one mask
            _check_part(chk, f"cfg {cfg} shared", part.sum(0), dx, tails[0], name)
        else:
            for z in range(2):
                _check_part(chk, f"cfg {cfg} group {z}", part[z].sum(0), dx[z], tails[z], name)
        _tickets_zero(chk, f"cfg {cfg}", call)
    chk.done()
    need = MIN_RAN[family] if family in MIN_RAN else MIN_RAN_PATCH[(family, Co)]
    assert ran >= need, (ran, need)


@pytest.mark.parametrize("family", FAMILIES)
def test_join_narrow_tail_and_replicas(fn, tails, family):
    """Case 4: a 48-channel gradient feeding a 32-channel tail (channels 32-47 get the plain sum), part between
    guard bands.  Case 5: pnrep = 4 -- replica rows 4 and above stay exactly zero."""
    from mtl_das_pytorch_amd.engine import guard
    Co = 32 if family == "patch_persistent" else 48
    wide, conv, tail, chk, ran = Conv(400, 48, Co, 3, 1, 1, 1), Conv(500, C, Co, 3, 1, 1, 1), tails[0], Checker(), 0
    was = guard.enabled()
    guard.enable(True)
    try:
        for cfg in _families(fn)[family]:
            part = guard.alloc((NREP, 3, C), torch.float64, "cuda", zero=True, label="narrow tail part")
            call = _prepare(fn, wide.dy.cuda(), wide.w.cuda(), (H, W), 1, 1, cfg=cfg, add=wide.dsrcs,
                            bn_stats=_bnb(fn, tail, "relu", part, C=C))
            if call is None:
                continue
            dx = call.run()
            ran += 1
            chk.elementwise(f"cfg {cfg} narrow", dx, wide.g(1))
            _check_part(chk, f"cfg {cfg} narrow", part.sum(0), dx[..., :C], tail, "relu")
            _tickets_zero(chk, f"cfg {cfg} narrow", call)

            part = guard.alloc((NREP, 3, C), torch.float64, "cuda", zero=True, label="pnrep 4 part")
            call = _prepare(fn, conv.dy.cuda(), conv.w.cuda(), (H, W), 1, 1, cfg=cfg, add=conv.dsrcs,
                            bn_stats=_bnb(fn, tail, "add", part, bn=bn_of(fn, tail, pnrep=4)))
            dx = call.run()
            chk.elementwise(f"cfg {cfg} pnrep", dx, conv.g(1))
            chk.true(f"cfg {cfg} replica rows >= 4 zero", bool((part[4:] == 0).all()))
            _check_part(chk, f"cfg {cfg} pnrep", part[:4].sum(0), dx, tail, "add")
            torch.cuda.synchronize()
            bad = guard.check()
            guard.reset()
            chk.true(f"cfg {cfg} guard bands {bad}", not bad)
    finally:
        guard.reset()
        guard.enable(was)
    chk.done()
    need = MIN_RAN[family] if family in MIN_RAN else MIN_RAN_PATCH[(family, Co)]
    assert ran >= need, (ran, need)


def test_parse_conv_rejections(fn, tails):
    """The binding refuses launch arguments the epilogue cannot honour (parsed, never launched)."""
    from mtl_das_pytorch_amd.ops.hip import lib
    conv, tail = Conv(600, C, 48, 3, 1, 1, 3), tails[0]
    part = torch.zeros(NREP, 3, C, device="cuda", dtype=torch.float64)

    def base():
        return fn.prepare_conv2d_dgrad(conv.dy.cuda(), conv.w.cuda(), (H, W), 1, 1, cfg=1, add=conv.dsrcs,
                                       bn_stats=_bnb(fn, tail, "add", part)).d

    def refused(d, mode=1):
        with pytest.raises(RuntimeError):
            lib().conv_workspace(mode, fn.lds_cfg(0), 1, d)

    lib().conv_workspace(1, fn.lds_cfg(0), 1, base())  # the unmodified arguments parse
    d = base()
    d["add"] = d["add"] + [dict(d["add"][1])]
    refused(d)                                         # more than 3 sources
    d = base()
    d["add"][1]["ld"] = C - 4
    refused(d)                                         # pitch below N
    d = base()
    d["add"][0]["ld"] = 66
    refused(d)                                         # pitch not a multiple of 4
    for Cbad in (28, C + 8):                           # C % 8, C > N
        d = base()
        d["bnb"]["C"] = Cbad
        d["bnb"]["bn"] = dict(d["bnb"]["bn"], C=Cbad)
        refused(d)
    d = base()
    d["bnb"].update(pgs=0, ygs=8)
    refused(d)                                         # a shared tail with a per-group y
    d["bnb"].update(ygs=0)
    lib().conv_workspace(1, fn.lds_cfg(0), 1, d)
    d = base()
    d["bnb"]["bn"] = dict(d["bnb"]["bn"], training=0)
    refused(d)                                         # eval-mode BN
    x = torch.zeros(B, H, W, C, device="cuda", dtype=torch.bfloat16)
    for key in ("add", "bnb"):                         # either on a forward launch
        f = fn.prepare_conv2d(x, torch.zeros(C, C, 3, 3, device="cuda"), padding=1, cfg=1).d
        lib().conv_workspace(0, fn.lds_cfg(0), 1, f)
        f[key] = base()[key]
        refused(f, mode=0)


# ---------------------------------------------------------------------------------------------------
# B. BN tail backward modes
def _sources(t, name, n, seed):
    """``n`` bf16 gradient sources on the tail's output grid (CPU) and their device forms with mixed pitches."""
    Bb, Hh, Ww, Cc = t.t["y"].shape
    if name == "pool":
        Hh, Ww = (Hh + 1) // 2, (Ww + 1) // 2
    gen = torch.Generator().manual_seed(seed)
    cpu = [torch.randn(Bb, Hh, Ww, Cc, generator=gen).bfloat16() for _ in range(n)]
    return cpu, [s.cuda() if i % 3 == 0 else sliced(s, Cc + 8 * (i % 3), 8 * (i % 2)) for i, s in enumerate(cpu)]


def _run_tail(fn, t, name, dev_srcs, bn=None, bn2=None, **kw):
    kind, proj = R.KINDS[name]
    Cc = t.t["y"].shape[-1]
    par = [torch.full((Cc,), float("nan"), device="cuda") for _ in range(4)]
    res = fn.bn_tail_backward(kind, t.dev["y"], bn or bn_of(fn, t), dev_srcs, par[0], par[1], r=t.r(name),
                              bn2=(bn2 or bn_of(fn, t, "2")) if proj else None, dgamma2=par[2], dbeta2=par[3], **kw)
    return res, par


def _check_tail(chk, what, name, ref, res, par, gscale=1.0):
    """Outputs of a tail backward against the reference ``ref`` (bwd_ref.tail of the same sources)."""
    kind, proj = R.KINDS[name]
    dy, side, dy2 = res
    chk.l2("dy", what, dy, ref["dy"], TOL_ACT)
    amb = ref["amb"]

    def ambt(f):
        if amb is None:
            return None
        return (ref["gfull"] * f).abs() * amb.double()
    one = torch.ones_like(ref["dz"])
    chk.sums(what + " dbeta", par[1].cpu() / gscale, ref["dz"], ambt(one))
    chk.sums(what + " dgamma", par[0].cpu() / gscale, ref["dz"] * ref["xhat"], ambt(ref["xhat"]))
    if proj:
        chk.l2("dy2", what, dy2, ref["dy2"], TOL_ACT)
        chk.sums(what + " dbeta2", par[3].cpu() / gscale, ref["dz"], ambt(one))
        chk.sums(what + " dgamma2", par[2].cpu() / gscale, ref["dz"] * ref["xhat2"], ambt(ref["xhat2"]))
    elif side is not None:
        chk.l2("side", what, side, ref["side"], TOL_ACT)


def _ref_tail(t, name, cpu_srcs, gscale=1.0):
    ref = R.kind_tail(name, t.t, cpu_srcs, gscale)
    g = sum(s.double() for s in cpu_srcs)
    ref["gfull"] = R.up(g, *t.t["y"].shape[1:3]) if name == "pool" else g  # |term| of an element whose mask flips
    return ref


SRC_INPUTS = R.TAIL_INPUTS[:3]


@pytest.mark.parametrize("name", list(R.KINDS))
@pytest.mark.parametrize("inp", SRC_INPUTS, ids=lambda i: f"C{i[4]}")
def test_tail_sources(fn, inp, name):
    """2, 4 and 6 gradient sources with mixed pitches through reduce + apply, with and without the stored dz; the
    statistics come from the unrounded sum of the sources (reference: the fp64 sum of the bf16 sources)."""
    seed, Bb, Hh, Ww, Cc, _ = inp
    t, chk = Tail(seed, (Bb, Hh, Ww), Cc), Checker()
    for n in (2, 4, 6):
        cpu, dev = _sources(t, name, n, seed + n)
        ref = _ref_tail(t, name, cpu)
        for store_dz in (False, True):
            res, par = _run_tail(fn, t, name, dev, store_dz=store_dz)
            _check_tail(chk, f"{n} sources store_dz={store_dz}", name, ref, res, par)
    chk.done()


@pytest.mark.parametrize("name", list(R.KINDS))
@pytest.mark.parametrize("inp", SRC_INPUTS, ids=lambda i: f"C{i[4]}")
def test_tail_subset_reduce_then_apply(fn, inp, name):
    """The SyncBN composition: reduce-only (fused = 3) over two of four sources, the other two sources' share of the
    sums added into part by hand, then apply-only (fused = 2) over all four with gscale = 0.5."""
    seed, Bb, Hh, Ww, Cc, _ = inp
    t, chk = Tail(seed, (Bb, Hh, Ww), Cc), Checker()
    proj = R.KINDS[name][1]
    cpu, dev = _sources(t, name, 4, seed + 100)
    part = torch.zeros(NREP, 3, Cc, device="cuda", dtype=torch.float64)
    res, _ = _run_tail(fn, t, name, dev[:2], fused=3, part=part)
    assert res == (None, None, None)
    rest = R.kind_tail(name, t.t, cpu[2:])
    part[0, 0] += rest["sdz"].cuda()
    part[0, 1] += rest["sdzx"].cuda()
    if proj:
        part[0, 2] += rest["sdzx2"].cuda()
    res, par = _run_tail(fn, t, name, dev, part=part, gscale=0.5)
    _check_tail(chk, "subset reduce + apply", name, _ref_tail(t, name, cpu, 0.5), res, par, gscale=0.5)
    chk.done()
    with pytest.raises(RuntimeError, match="rc=-5"):  # apply-only recomputes dz: no stored-dz form
        _run_tail(fn, t, name, dev, part=part, store_dz=True)
    with pytest.raises(RuntimeError, match="rc=-5"):  # the single-launch kernel does not scale its sums
        _run_tail(fn, t, name, dev, fused=1, gscale=0.5)


@pytest.mark.parametrize("name", list(R.KINDS))
def test_tail_groups(fn, name):
    """G = 2 with distinct inputs and BN parameters per group."""
    ts = [Tail(i[0], i[1:4], i[4]) for i in R.TAIL_INPUTS[3:5]]
    kind, proj = R.KINDS[name]
    Cc, chk = ts[0].t["y"].shape[-1], Checker()
    srcs = [_sources(t, name, 2, 50 + z) for z, t in enumerate(ts)]
    dev = [torch.stack([srcs[z][0][i] for z in range(2)]).cuda() for i in range(2)]
    par = [torch.full((2, Cc), float("nan"), device="cuda") for _ in range(4)]
    r = torch.stack([t.r(name) for t in ts]) if ts[0].r(name) is not None else None
    res = fn.bn_tail_backward(kind, torch.stack([t.dev["y"] for t in ts]), bn_of(fn, ts), dev, par[0], par[1], r=r,
                              bn2=bn_of(fn, ts, "2") if proj else None, dgamma2=par[2], dbeta2=par[3], groups=2)
    for z, t in enumerate(ts):
        _check_tail(chk, f"group {z}", name, _ref_tail(t, name, srcs[z][0]),
                    tuple(None if o is None else o[z] for o in res), [p[z] for p in par])
    chk.done()


@pytest.mark.parametrize("inp", R.TAIL_INPUTS[5:8], ids=lambda i: f"M{i[1] * i[2] * i[3]}")
def test_tail_single_launch(fn, inp):
    """The single-launch kernel (fused = 1) at its register depths R = 1, 2, 4 (1024, 2048, 4096 pixels; the
    residual kinds take at most R = 2)."""
    seed, Bb, Hh, Ww, Cc, kinds = inp
    t, chk = Tail(seed, (Bb, Hh, Ww), Cc), Checker()
    for name in kinds:
        cpu, dev = _sources(t, name, 2, seed + 7)
        res, par = _run_tail(fn, t, name, dev, fused=1)
        _check_tail(chk, name, name, _ref_tail(t, name, cpu), res, par)
    chk.done()


def test_tail_pool_odd_windows(fn):
    """POOL_RELU with odd H and W: the last row and column of windows are ceil-mode partial windows."""
    seed, Bb, Hh, Ww, Cc, _ = R.TAIL_INPUTS[8]
    assert Hh % 2 and Ww % 2
    t, chk = Tail(seed, (Bb, Hh, Ww), Cc), Checker()
    cpu, dev = _sources(t, "pool", 2, seed + 1)
    ref = _ref_tail(t, "pool", cpu)
    for store_dz in (False, True):
        res, par = _run_tail(fn, t, "pool", dev, store_dz=store_dz)
        _check_tail(chk, f"store_dz={store_dz}", "pool", ref, res, par)
    chk.done()
