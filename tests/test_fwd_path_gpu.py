"""The forward path at kernel level against the fp64 references of tests/fwd_ref.py (themselves checked on the CPU,
with the sensitivity of every checker used here, by tests/test_fwd_ref.py).

A. The forward epilogue of every conv kernel family (csrc/conv.hip conv_igemm at both pipeline depths,
   csrc/conv_lds.hip LDS with K splits 1 and 2 / LDS-DMA in both rings / patch / persistent patch) on INTEGER data:
   the stored y equals bf16_rne(ref) bit for bit and the replica rows sum to the exact fp64 sum(y), sum(y^2) of the
   unrounded y; NaN in every input column and gap the conv may not read, a sentinel in every output column, gap and
   guard row it may not write; strides, 1x1 / 5x5 / 1x7 / 7x1, the valid form, two input segments, G = 3 with gaps,
   the output as a column slice, no bias, no statistics.
B. Statistics plumbing: stats_nrep, the CONV_XCD tile order, BNArgs::nrep, BNArgs::sld (one conv feeding two BNs).
C. Normalise-on-load forward (training, eval, groups, a large shift on padded borders), refused by the LDS-DMA and
   the persistent patch kernels.
D. The BN forward tails of csrc/bn.hip: published constants, running statistics, all kinds, eval mode, batched.

The conv and tail launches go through ops/functional.py, whose prepare_conv2d / bn_args / bn_tail were extended
for this (groups, pitched inputs, ``out=`` slices, stats_nrep, sld + channel offset); the batched tail builds its
job dicts with functional.tail_fwd_args and its table with lib().tail_table, as the engine does.

Minimum configs per family (derived from the constraints in csrc/kernels.h and csrc/conv_lds.hip, ``min_ran``): every
implicit-GEMM config takes every geometry here (the LDS tiles need at most 2 (BM + BN) KC 2 = 96 KB, the LDS-DMA
rings at most 3 x 384 x 128 B = 144 KB + tables, below the 160 KB limit): igemm 14, igemm_deep 14, lds 30 (8 tiles x
KC 64 / 128 without the 128 x 128 tile at KC 128, x 2 splits), glds 28 (8 tiles + the 6 with a deep ring, x 2
splits).  The patch kernels take 3x3 / stride 1 with Wo <= BM and a channel slice cb in {16, 32, 64} dividing Cs (and
C0 of a two-segment input): Cs = 32 gives the 5 tiles x cb 16, 32 = 10; the persistent form holds one slice (Cs ==
cb): 5.

Bounds (none derived from what the kernels give):
  integer conv    y, sum(y), sum(y^2): ``==``.
  randn conv      y: 2^-8 |ref| + 1e-5 max|ref| (one bf16 ulp).  Statistics per channel against the fp64 sums of the
                  exact reference: with n pixels, K products per output, T = conv(|x|, |w|) + |b|, delta = K 2^-24 T,
                  |d sum(y)| <= sum(delta) + n 2^-24 sum|ref|, |d sum(y^2)| <= sum(2 |ref| delta + delta^2) +
                  (n + 1) 2^-24 sum(ref^2): the kernel's side is an fp32 accumulation of K products per element and an
                  fp32 sum of at most n values (then fp64), the reference's side is exact.
  constants       mean 2^-24 |mean|; invstd 4 2^-24 relative (the cast of var, the + eps rounding, rsqrtf at 1 ulp);
                  scale 5 2^-24 relative; shift 8 2^-24 (|beta| + |mean scale|).
  running stats   4 2^-24 (|(1 - m) old| + |m new|), m and eps as fp32.
  tail outputs    against fwd_ref.tail_fwd fed the kernel's own published fp32 constants: one bf16 ulp.
  NOL y_out       one bf16 ulp + sum over the ambiguous operands in the receptive field of |w| ulp_bf16(a) (operands
                  within 2^-21 relative of a bf16 rounding boundary, where a fused and an unfused fp32 evaluation may
                  differ); eval mode, whose constants are not published, adds the constants' own bounds to the margin.

Worst observed values on MI355X (printed by every test, ``Checker.done``), as err / bound:
  integer conv    0 mismatching elements in y, sum(y), sum(y^2) over every config of every family and every case; every
                  sentinel intact, every output finite, every split-K ticket back at zero.
  randn conv      y 0.986; sum(y) 3.6e-4, sum(y^2) 4.7e-4 (the bound is a worst case, the errors average out).
  constants       mean 0.991 (a half-ulp rounding, at most 1 by construction), invstd 0.423 (rsqrtf stays within its
                  documented accuracy: 1.7 of the 4 units), scale 0.474, shift 0.379.
  running stats   run_mean 0.470, run_var 0.634.
  tail outputs    0.991 (one bf16 ulp next to a rounding boundary); batched == single launches bit for bit.
  NOL             y_out 0.990 (training) / 0.986 (eval); sum(y) 0.061, sum(y^2) 0.056; ambiguous share <= 1 %.
  Every family ran the configs its minimum names.  No kernel read a foreign column or a gap (the NaN poison never
  reached an output) and no kernel, binding or host function had to change; ops/functional.py was extended only.
"""
import pytest
import torch

import fwd_ref as R
from test_bwd_join_gpu import FAMILIES, GEMM_FAMILIES, _families
from wpath_ref import NAN, SENT

pytestmark = pytest.mark.gpu

NREP = 32
NOL_FAMILIES = ["igemm", "igemm_deep", "lds", "patch"]
EXPECT_3X3 = {"igemm": 14, "igemm_deep": 14, "lds": 30, "glds": 28, "patch": 10, "patch_persistent": 5}
KINDS = {"none": (R.ACT_NONE, False), "relu": (R.ACT_RELU, False), "sigmoid": (R.ACT_SIGMOID, False),
         "sigmul": (R.SIGMUL, False), "add": (R.ADD_RELU, False), "add_proj": (R.ADD_RELU, True),
         "pool": (R.POOL_RELU, False)}
HYPER = [(0.1, 1e-5), (0.25, 1e-3)]   # (momentum, eps)


@pytest.fixture(scope="module")
def fn():
    from mtl_das_pytorch_amd.ops import functional as fn
    return fn


def min_ran(fn, family, c):
    """Configs of ``family`` that must accept case ``c`` (see the module docstring)."""
    if family in GEMM_FAMILIES:
        return len(_families(fn)[family])
    if (c.KH, c.KW, c.sh, c.sw) != (3, 3, 1, 1):
        return 0
    cbs = [cb for cb in fn.PATCH_CB if c.Cs % cb == 0 and (c.C1 == 0 or c.C0 % cb == 0)]
    if family == "patch_persistent":
        cbs = [cb for cb in cbs if cb == c.Cs]
    return len(fn.PATCH_TILES) * len(cbs)


def test_minimum_config_counts(fn):
    c = R.FCASE["3x3 p1"]
    assert (c.Cs, c.Co) == (32, 48)
    assert {f: min_ran(fn, f, c) for f in FAMILIES} == EXPECT_3X3
    assert c.M == 1428 and all(c.M % bm for bm in (16, 32, 64, 128, 256)) and all(c.Co % bn for bn in (32, 64, 128))


# ---------------------------------------------------------------------------------------------------
# conv problems
class Problem:
    """Device copies of one case's inputs and its reference (computed once per module)."""

    def __init__(self, c):
        self.c = c
        inp = R.conv_inputs(c)
        self.ref = R.conv_fwd(c, inp)
        self.inp = inp
        self.buf0 = inp["buf0"].cuda()
        self.buf1 = inp["buf1"].cuda() if c.C1 else None
        self.w = inp["w"].cuda()
        self.b = inp["b"].cuda() if inp["b"] is not None else None
        self.out0 = R.out_buf(c).cuda()
        self.dref = {k: self.ref[k].cuda() for k in ("ybf", "s1", "s2")}


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(R.FCASE[name])
    return _problems[name]


def launch(fn, P, cfg, stats=True, nrep=None, nol=None):
    """One forward launch of problem ``P`` into a fresh sentinel-filled output buffer: (flat output buffer, replica
    rows [G, NREP, 2, Co] or None, the prepared call), or None when the config does not take the geometry."""
    c = P.c
    flat = P.out0.clone()
    out = R.out_view(flat, c)
    st = torch.zeros(c.G, NREP, 2, c.Co, device="cuda", dtype=torch.float64) if stats else None
    x = R.in_view(P.buf0, c)
    x2 = R.in_view(P.buf1, c, 1) if c.C1 else None
    w, b = P.w, P.b
    one = c.G == 1   # the ungrouped form of the API

    def sq(t):
        return t[0] if (one and t is not None) else t
    try:
        call = fn.prepare_conv2d(sq(x), sq(w), sq(b), (c.sh, c.sw), (c.ph, c.pw), stats=sq(st), x2=sq(x2), cfg=cfg,
                                 nol=nol, groups=None if one else c.G, out=sq(out), stats_nrep=nrep)
    except ValueError:
        return None
    call.run()
    return flat, st, call


def tickets_zero(chk, what, call):
    if call._ws:
        chk.true(what + " split-K tickets", int(call._ws[1].abs().sum()) == 0)


# ---------------------------------------------------------------------------------------------------
# A. conv forward epilogue, integer data
@pytest.mark.parametrize("name", [c.name for c in R.FCASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_conv_epilogue_exact(fn, family, name):
    P, chk, ran = problem(name), R.Checker(), 0
    for cfg in _families(fn)[family]:
        res = launch(fn, P, cfg)
        if res is None:
            continue
        ran += 1
        flat, st, call = res
        chk.conv_exact(f"cfg {cfg}", P.c, flat, st, P.dref)
        tickets_zero(chk, f"cfg {cfg}", call)
    chk.done()
    assert ran >= min_ran(fn, family, P.c), (ran, min_ran(fn, family, P.c))


@pytest.mark.parametrize("family", FAMILIES)
def test_conv_without_statistics(fn, family):
    """Bias, no statistics: y as before, and a replica buffer the launch was not given stays untouched."""
    P, chk, ran = problem("3x3 p1"), R.Checker(), 0
    poison = torch.full((NREP, 2, P.c.Co), SENT, device="cuda", dtype=torch.float64)
    for cfg in _families(fn)[family]:
        res = launch(fn, P, cfg, stats=False)
        if res is None:
            continue
        ran += 1
        chk.conv_exact(f"cfg {cfg}", P.c, res[0], None, P.dref)
        chk.sentinels(f"cfg {cfg} replicas", poison)
        tickets_zero(chk, f"cfg {cfg}", res[2])
    chk.done()
    assert ran >= EXPECT_3X3[family], ran


@pytest.mark.parametrize("name", [c.name for c in R.RCASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_conv_randn(fn, family, name):
    """The non-integer path: y by the one-ulp bound, the statistics by the accumulation bound of the docstring."""
    P, chk, ran = problem(name), R.Checker(), 0
    c = P.c
    b1, b2 = R.randn_stat_bounds(c, P.ref)
    for cfg in _families(fn)[family]:
        res = launch(fn, P, cfg)
        if res is None:
            continue
        ran += 1
        flat, st, call = res
        chk.act(f"cfg {cfg} y", R.out_view(flat, c), P.ref["y"], kind="conv y")
        chk.sentinels(f"cfg {cfg} output sentinels", R.out_foreign(flat, c))
        chk.bounded("sum(y)", f"cfg {cfg}", st[:, :, 0].sum(1), P.ref["s1"], b1)
        chk.bounded("sum(y^2)", f"cfg {cfg}", st[:, :, 1].sum(1), P.ref["s2"], b2)
        tickets_zero(chk, f"cfg {cfg}", call)
    chk.done()
    assert ran >= min_ran(fn, family, c), ran


# ---------------------------------------------------------------------------------------------------
# B. statistics plumbing
@pytest.mark.parametrize("nrep", [1, 4, 32])
@pytest.mark.parametrize("family", FAMILIES)
def test_stats_nrep(fn, family, nrep):
    """ConvArgs::stats_nrep: rows >= stats_nrep stay zero, the totals are unchanged."""
    P, chk, ran = problem("3x3 p1"), R.Checker(), 0
    for cfg in _families(fn)[family]:
        res = launch(fn, P, cfg, nrep=nrep)
        if res is None:
            continue
        ran += 1
        chk.conv_exact(f"cfg {cfg} nrep {nrep}", P.c, res[0], res[1], P.dref, nrep=nrep)
    chk.done()
    assert ran >= EXPECT_3X3[family], ran


@pytest.mark.parametrize("name", ["3x3 p1", "G3 gaps"])
@pytest.mark.parametrize("family", FAMILIES)
def test_xcd_order(fn, family, name):
    """The CONV_XCD tile order: y bitwise equal to the plain order, the totals equal (one config per family: the
    first and the last that take the case)."""
    P, chk = problem(name), R.Checker()
    cfgs = [cfg for cfg in _families(fn)[family] if launch(fn, P, cfg) is not None]
    assert cfgs
    for cfg in {cfgs[0], cfgs[-1]}:
        plain, xcd = launch(fn, P, cfg), launch(fn, P, cfg | fn.CONV_XCD)
        chk.bits(f"cfg {cfg} y", xcd[0], plain[0])
        chk.conv_exact(f"cfg {cfg} xcd", P.c, xcd[0], xcd[1], P.dref)
        tickets_zero(chk, f"cfg {cfg} xcd", xcd[2])
    chk.done()


# ---------------------------------------------------------------------------------------------------
# BN state of a tail / a normalise-on-load conv
class BN:
    """Device parameters, state and replica rows of one BN ([G, C]; ``grouped`` False: the ungrouped API forms) and
    the fp64 reference of what a training launch must leave behind."""

    def __init__(self, fn, y, gamma, beta, rm, rv, momentum=0.1, eps=1e-5, nrep=NREP, training=True, fill=0.0,
                 grouped=False, seed=0, stats=None, sld=None, coff=0, tot=None):
        G, C = gamma.shape
        self.G, self.C, self.n = G, C, y[0].numel() // C if y is not None else None
        self.momentum, self.eps, self.training = momentum, eps, training
        self.gamma, self.beta, self.rm0, self.rv0 = gamma, beta, rm, rv
        self.tot = R.totals(y) if tot is None else tot
        if stats is None:
            rep = R.spread(self.tot, nrep, NREP, seed, fill)
            self.tot = rep[:, :nrep].sum(1)      # the replica rows' own fp64 sum
            if not training:
                rep.fill_(fill)                  # eval mode reads no replica row
            stats = rep.cuda()
        self.stats = stats
        self.rm, self.rv = rm.clone().cuda(), rv.clone().cuda()
        self.nbt = torch.zeros(G, dtype=torch.int64, device="cuda")
        self.consts = torch.full((G, 4, C), SENT, device="cuda")
        self.dgamma, self.dbeta = gamma.cuda(), beta.cuda()
        sq = (lambda t: t) if grouped else (lambda t: t[0])
        self.args = fn.bn_args(sq(stats), sq(self.dgamma), sq(self.dbeta), sq(self.rm), sq(self.rv), self.nbt,
                               count=self.n, eps=eps, momentum=momentum, training=training, consts=self.consts,
                               nrep=nrep, sld=sld, coff=coff)

    def set_count(self, n):
        self.n = n
        self.args["count"] = n

    def check_training(self, chk, what, launches=1):
        """Published constants, running statistics, nbt after ``launches`` = 1 training launch; returns the
        kernel's constants (CPU, [G, 4, C])."""
        k = self.consts.cpu()
        ref, var = R.bn_consts(self.tot, self.n, self.gamma, self.beta, R.f32(self.eps))
        chk.true(what + " consts written", bool(torch.isfinite(k).all()) and not bool((k == SENT).any()))
        chk.consts(what, k, ref, self.beta)
        chk.running_stats(what, self.rm.cpu(), self.rv.cpu(), self.rm0, self.rv0, ref[:, 2], var, self.n,
                          self.momentum)
        chk.exact(what + " nbt", self.nbt, torch.full((self.G,), launches, dtype=torch.int64))
        return k

    def check_eval(self, chk, what):
        """Eval mode: state bit-unchanged, consts unwritten; returns the fp64 reference constants."""
        chk.bits(what + " run_mean", self.rm, self.rm0)
        chk.bits(what + " run_var", self.rv, self.rv0)
        chk.exact(what + " nbt", self.nbt, torch.zeros(self.G, dtype=torch.int64))
        chk.sentinels(what + " consts", self.consts)
        return R.eval_consts(self.rm0, self.rv0, self.gamma, self.beta, R.f32(self.eps))


# ---------------------------------------------------------------------------------------------------
# C. normalise-on-load forward
_nol_refs = {}


def nol_reference(c, d, k, kind, slack=None):
    """(ref [G, B, Ho, Wo, Co], extra bound, T) from constants ``k`` [G, 4, Cs] (fp64 on the CPU), cached by their
    bits: the conv of the operand, the slack of its ambiguous elements, conv(|a|, |w|)."""
    key = (c.name, kind, k.numpy().tobytes(), slack is not None)
    if key not in _nol_refs:
        refs, extras, Ts, shares = [], [], [], []
        for z in range(c.G):
            a, amb = R.nol_operand(d["y"][z], k[z, 0], k[z, 1], kind, slack=0.0 if slack is None else slack[z])
            ref, extra = R.nol_conv(a, amb, d["w"][z], c)
            refs.append(ref)
            extras.append(extra)
            Ts.append(R.conv2d_nhwc(a.abs(), d["w"][z].abs(), None, c))
            shares.append(float(amb.double().mean()))
        _nol_refs[key] = (torch.stack(refs), torch.stack(extras), torch.stack(Ts), max(shares))
    return _nol_refs[key]


class NolProblem:
    """Device copies of a normalise-on-load case's inputs, in the form ``launch`` takes."""

    def __init__(self, c, d):
        self.c, self.buf0, self.buf1, self.w, self.b = c, d["buf0"].cuda(), None, d["w"].cuda(), None
        self.out0 = R.out_buf(c).cuda()


def nol_bn(fn, c, d, training=True, momentum=0.1, eps=1e-5):
    return BN(fn, d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], momentum, eps, nrep=8, training=training,
              fill=0.0 if training else NAN, grouped=c.G > 1, seed=c.seed)


@pytest.mark.parametrize("name", [c.name for c in R.NCASES])
@pytest.mark.parametrize("family", NOL_FAMILIES)
def test_nol_training(fn, family, name):
    """Training-mode normalise-on-load: the published constants, the running statistics, nbt == 1 per group, y_out
    against the fp64 conv of the operand built from the kernel's own constants, the statistics of y_out."""
    c = R.FCASE[name]
    d = R.nol_inputs(c, big_shift="big shift" in name)
    P = NolProblem(c, d)
    chk, ran = R.Checker(), 0
    for i, cfg in enumerate(_families(fn)[family]):
        for kind in (R.ACT_NONE, R.ACT_RELU):
            momentum, eps = HYPER[(i + kind) % 2]
            bn = nol_bn(fn, c, d, True, momentum, eps)
            res = launch(fn, P, cfg, nol=(bn.args, kind))
            if res is None:
                break
            ran += kind == R.ACT_RELU   # once per config
            flat, st, call = res
            what = f"cfg {cfg} kind {kind}"
            k = bn.check_training(chk, what).double()
            ref, extra, T, share = nol_reference(c, d, k, kind)
            chk.true(what + " ambiguous share", share <= 0.01)
            chk.act(what + " y_out", R.out_view(flat, c), ref, extra, kind="nol y_out")
            chk.sentinels(what + " output sentinels", R.out_foreign(flat, c))
            b1, b2 = R.randn_stat_bounds(c, {"y": ref, "T": T})
            red = (1, 2, 3)
            chk.bounded("nol sum(y)", what, st[:, :, 0].sum(1), ref.sum(red), b1 + extra.sum(red))
            chk.bounded("nol sum(y^2)", what, st[:, :, 1].sum(1), (ref * ref).sum(red),
                        b2 + (2 * ref.abs() * extra + extra * extra).sum(red))
            tickets_zero(chk, what, call)
    chk.done()
    need = min_ran(fn, family, c)
    assert ran >= need, (ran, need)


@pytest.mark.parametrize("name", ["nol 3x3", "nol 3x3 G2"])
@pytest.mark.parametrize("family", NOL_FAMILIES)
def test_nol_eval(fn, family, name):
    """Eval-mode normalise-on-load: running statistics and nbt bit-unchanged, no constants published, the (NaN)
    replica rows not read; y_out against the operand of the fp64 running-statistics constants, whose ambiguity margin
    carries the constants' own fp32 bounds (they are not published)."""
    c = R.FCASE[name]
    d = R.nol_inputs(c)
    P = NolProblem(c, d)
    chk, ran = R.Checker(), 0
    for cfg in _families(fn)[family]:
        for kind in (R.ACT_NONE, R.ACT_RELU):
            bn = nol_bn(fn, c, d, training=False)
            res = launch(fn, P, cfg, nol=(bn.args, kind))
            if res is None:
                break
            ran += kind == R.ACT_RELU   # once per config
            what = f"cfg {cfg} kind {kind}"
            k = bn.check_eval(chk, what)
            sc, sh, mu = (k[:, i][:, None, None, None] for i in range(3))
            slack = 2.0 ** -24 * (5 * (d["y"].double() * sc).abs() + 8 * (d["beta"].double()[:, None, None, None].abs()
                                                                         + (mu * sc).abs()))
            ref, extra, _, share = nol_reference(c, d, k, kind, slack)
            chk.true(what + " ambiguous share", share <= 0.01)
            chk.act(what + " y_out", R.out_view(res[0], c), ref, extra, kind="nol eval y_out")
            chk.sentinels(what + " output sentinels", R.out_foreign(res[0], c))
    chk.done()
    assert ran >= min_ran(fn, family, c), ran


@pytest.mark.parametrize("family", ["glds", "patch_persistent"])
def test_nol_refused(fn, family):
    """MODE_FWD_NOL is refused by the LDS-DMA kernels and the persistent patch form (no on-load transform)."""
    c = R.FCASE["nol 3x3"]
    d = R.nol_inputs(c)
    P = NolProblem(c, d)
    bn = nol_bn(fn, c, d)
    plain = 0
    for cfg in _families(fn)[family]:
        assert launch(fn, P, cfg, nol=(bn.args, R.ACT_RELU)) is None, cfg
        plain += launch(fn, P, cfg) is not None
    assert plain >= EXPECT_3X3[family]   # ... although the geometry itself is theirs
    assert int(bn.nbt.sum()) == 0


# ---------------------------------------------------------------------------------------------------
# D. BN forward tails
def sliced(t, pad, off, fill):
    """``t`` [..., C] as the column slice [off, off + C) of a device buffer of pitch C + pad filled with ``fill``;
    returns (slice, buffer)."""
    C = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + (C + pad,), fill, dtype=t.dtype, device="cuda")
    buf[..., off:off + C] = t.cuda()
    return buf[..., off:off + C], buf


def foreign_cols(buf, off, C):
    return torch.cat([buf[..., :off].reshape(-1), buf[..., off + C:].reshape(-1)])


_tail_inputs = {}


def tail_inputs(seed, shape, C, G=1):
    key = (seed, shape, C, G)
    if key not in _tail_inputs:
        _tail_inputs[key] = R.tail_y(seed, shape, C, G)
    return _tail_inputs[key]


_tail_refs = {}


def tail_reference(key, kind, proj, d, k, k2):
    """fp64 tail output [G, ...] from constants [G, 4, C] (CPU), cached by their bits."""
    key = key + (kind, proj, k.numpy().tobytes(), k2.numpy().tobytes() if proj else b"")
    if key not in _tail_refs:
        r = d["y2"] if proj else d["r"]
        _tail_refs[key] = torch.stack([R.tail_fwd(kind, d["y"][z], k[z].double(), r[z], k2[z].double() if proj else None)
                                       for z in range(d["y"].shape[0])])
    return _tail_refs[key]


def run_tail(fn, chk, what, key, d, name, blocks, momentum=0.1, eps=1e-5, nrep=NREP, fill=0.0, training=True,
             grouped=False, slices=True):
    """One forward tail launch on tail_y inputs ``d`` (y, r and the output as column slices between sentinels /
    NaN) and every check of its results; returns (output slice, bn, bn2)."""
    kind, proj = KINDS[name]
    G = d["y"].shape[0]
    mk = dict(momentum=momentum, eps=eps, nrep=nrep, training=training, fill=fill, grouped=grouped)
    bn = BN(fn, d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], seed=1, **mk)
    bn2 = BN(fn, d["y2"], d["gamma2"], d["beta2"], d["rm2"], d["rv2"], seed=2, **mk) if proj else None
    pad = 16 if slices else 0
    y, _ = sliced(d["y"], pad, 8 if slices else 0, NAN)
    r = None
    if kind in (R.SIGMUL, R.ADD_RELU):
        r, _ = sliced(d["y2"] if proj else d["r"], 2 * pad, pad, NAN)
    Bb, Hh, Ww, C = d["y"].shape[1:]
    oshape = (G, Bb, (Hh + 1) // 2, (Ww + 1) // 2, C) if kind == R.POOL_RELU else tuple(d["y"].shape)
    out, obuf = sliced(torch.full(oshape, SENT).bfloat16(), pad, 8 if slices else 0, SENT)
    sq = (lambda t: t) if grouped else (lambda t: None if t is None else t[0])
    fn.bn_tail(kind, sq(y), bn.args, r=sq(r), bn2=bn2.args if proj else None, blocks=blocks,
               groups=G if grouped else None, out=sq(out))
    if training:
        k = bn.check_training(chk, what)
        k2 = bn2.check_training(chk, what + " (2)") if proj else None
    else:
        k = bn.check_eval(chk, what)
        k2 = bn2.check_eval(chk, what + " (2)") if proj else None
    ref = tail_reference(key, kind, proj, d, k, k2)
    chk.act(what + " out", out, ref, kind="tail out")
    chk.sentinels(what + " output sentinels", foreign_cols(obuf, 8 if slices else 0, C))
    return out, bn, bn2


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("C", [8, 48, 128, 448])
def test_tail_training(fn, C, name):
    """Every kind at C = 8 / 48 (idle threads) / 128 / 448 (the widest BN of the models) with 1, 3 and 64 blocks
    (the two-pixel loop without a second pixel, M odd against the step, more blocks than pixels at C = 8), both
    (momentum, eps) pairs, non-trivial running statistics."""
    d, chk = tail_inputs(C, R.BASE, C), R.Checker()
    for blocks in (1, 3, 64):
        for momentum, eps in HYPER:
            run_tail(fn, chk, f"blocks {blocks} m {momentum} eps {eps}", (C, R.BASE), d, name, blocks, momentum, eps)
    chk.done()


@pytest.mark.parametrize("name", list(KINDS))
def test_tail_small_map(fn, name):
    """(2, 9, 21) at C = 8: one block of 256 threads covers 32 pixel lanes, so 64 blocks outnumber the 378 pixels'
    steps (blocks without a pixel) and 3 blocks leave an odd remainder."""
    d, chk = tail_inputs(50, R.DEEP, 8), R.Checker()
    for blocks in (1, 3, 64):
        run_tail(fn, chk, f"blocks {blocks}", (50, R.DEEP), d, name, blocks, 0.25, 1e-3)
    chk.done()


@pytest.mark.parametrize("nrep", [1, 4])
@pytest.mark.parametrize("name", ["relu", "add_proj"])
def test_tail_nrep(fn, name, nrep):
    """BNArgs::nrep: replica rows >= nrep (1e30) are ignored."""
    d, chk = tail_inputs(48, R.BASE, 48), R.Checker()
    run_tail(fn, chk, f"nrep {nrep}", (48, R.BASE), d, name, 8, nrep=nrep, fill=1e30)
    chk.done()


@pytest.mark.parametrize("name", list(KINDS))
def test_tail_groups(fn, name):
    """G = 2 with [G, C] parameters, distinct inputs and state per group."""
    d, chk = tail_inputs(60, R.DEEP, 48, G=2), R.Checker()
    for blocks in (3, 16):
        run_tail(fn, chk, f"G2 blocks {blocks}", (60, R.DEEP, 2), d, name, blocks, 0.25, 1e-5, grouped=True)
    chk.done()


@pytest.mark.parametrize("shape", [R.BASE, R.DEEP, (1, 1, 6)], ids=str)
def test_tail_pool_shapes(fn, shape):
    """POOL_RELU on 17x42, 9x21 and 1x6: ceil-mode windows of one row / one column at the odd edges."""
    d, chk = tail_inputs(70, shape, 48), R.Checker()
    for blocks in (1, 5):
        run_tail(fn, chk, f"pool {shape} blocks {blocks}", (70, shape), d, "pool", blocks)
    chk.done()


def test_tail_count_one(fn):
    """count == 1: the variance is zero and run_var keeps the biased one (no division by count - 1)."""
    d, chk = tail_inputs(80, (1, 1, 1), 8), R.Checker()
    for name in ("none", "relu"):
        run_tail(fn, chk, name, (80, (1, 1, 1)), d, name, 1, 0.25, 1e-3)
    chk.done()


@pytest.mark.parametrize("name", list(KINDS))
def test_tail_eval(fn, name):
    """Eval mode: the outputs from the running statistics, the replica rows (1e30) not read, the state tensors
    bit-unchanged, consts unwritten."""
    d, chk = tail_inputs(48, R.BASE, 48), R.Checker()
    for blocks in (1, 64):
        run_tail(fn, chk, f"eval blocks {blocks}", (48, R.BASE), d, name, blocks, training=False, fill=1e30, nrep=4)
    chk.done()


def test_tail_two_bns_of_one_conv(fn):
    """BNArgs::sld: a Co = 48 conv's replica rows feed two tails, C = 16 at channel offset 0 and C = 32 at offset
    16, each reading its y as a slice of pitch 48."""
    P, chk = problem("3x3 p1"), R.Checker()
    c = P.c
    flat, st, _ = launch(fn, P, 1)
    chk.conv_exact("conv", c, flat, st, P.dref)
    y = R.out_view(flat, c)[0]
    ycpu = y.cpu()
    g = R.gen(90)
    for coff, C in ((0, 16), (16, 32)):
        par = [torch.rand(1, C, generator=g) + 0.5, 0.1 * torch.randn(1, C, generator=g),
               0.5 * torch.randn(1, C, generator=g), 0.5 + torch.rand(1, C, generator=g)]
        tot = torch.stack([P.ref["s1"][:, coff:coff + C], P.ref["s2"][:, coff:coff + C]], 1)
        bn = BN(fn, None, *par, momentum=0.25, stats=st, sld=c.Co, coff=coff, tot=tot)
        bn.set_count(c.M)
        ys = y[..., coff:coff + C]
        out = fn.bn_tail(R.ACT_RELU, ys, bn.args, blocks=7)
        k = bn.check_training(chk, f"C {C} at {coff}")
        # the kernel read the STORED bf16 y; its statistics are those of the unrounded y (the conv's)
        chk.act(f"C {C} at {coff} out", out, R.tail_fwd(R.ACT_RELU, ycpu[..., coff:coff + C], k[0].double()),
                kind="tail out")
    chk.done()


@pytest.mark.parametrize("kind", [R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID])
def test_tail_batched(fn, kind):
    """tail_fwd_batched: three jobs (C = 16, 48, 128; 1, 5, 64 blocks) writing adjacent column slices of one concat
    buffer with sentinel columns between and after them -- outputs, constants, running statistics and nbt bitwise
    equal to the three single launches (checked as every single launch is)."""
    from mtl_das_pytorch_amd.ops.hip import lib, stream
    name = {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_SIGMOID: "sigmoid"}[kind]
    chk = R.Checker()
    Cs, blocks = (16, 48, 128), (1, 5, 64)
    ds = [tail_inputs(100 + C, R.DEEP, C) for C in Cs]
    single = [run_tail(fn, chk, f"single C {C}", (100 + C, R.DEEP), d, name, b, 0.25, 1e-3)
              for C, d, b in zip(Cs, ds, blocks)]
    width = sum(Cs) + 8 * len(Cs)
    concat = torch.full((1,) + R.DEEP + (width,), SENT, device="cuda", dtype=torch.bfloat16)
    jobs, bns, outs, off = [], [], [], 0
    keep = []
    for C, d in zip(Cs, ds):
        bn = BN(fn, d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.25, 1e-3, seed=1)
        y, ybuf = sliced(d["y"], 16, 8, NAN)
        out = concat[..., off:off + C]
        args, _ = fn.tail_fwd_args(kind, y[0], bn.args, out=out[0])
        jobs.append(args)
        bns.append(bn)
        outs.append(out)
        keep.append(ybuf)
        off += C + 8
    raw, nblocks, max_c = lib().tail_table(jobs, list(blocks))
    assert nblocks == sum(blocks) and max_c == max(Cs)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    lib().tail_fwd_batched(kind, table.data_ptr(), len(jobs), nblocks, max_c, stream())
    torch.cuda.synchronize()
    mask = torch.ones(width, dtype=torch.bool, device="cuda")
    off = 0
    for C, bn, out, (sout, sbn, _) in zip(Cs, bns, outs, single):
        chk.bits(f"batched C {C} out", out.contiguous(), sout.contiguous())
        chk.bits(f"batched C {C} consts", bn.consts, sbn.consts)
        chk.bits(f"batched C {C} run_mean", bn.rm, sbn.rm)
        chk.bits(f"batched C {C} run_var", bn.rv, sbn.rv)
        chk.exact(f"batched C {C} nbt", bn.nbt, torch.ones(1, dtype=torch.int64))
        mask[off:off + C] = False
        off += C + 8
    chk.sentinels("concat sentinel columns", concat[..., mask])
    chk.done()
    for bad in (R.SIGMUL, R.ADD_RELU, R.POOL_RELU):   # a second operand or a pooled grid: not batched
        with pytest.raises(RuntimeError, match="rc=-1"):
            lib().tail_fwd_batched(bad, table.data_ptr(), len(jobs), nblocks, max_c, stream())
    for C, bn in zip(Cs, bns):
        assert int(bn.nbt[0]) == 1   # the refused launches ran nothing
