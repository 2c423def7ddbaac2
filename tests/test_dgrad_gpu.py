"""The data-gradient body of every conv kernel family against the fp64 scatter reference of tests/dgrad_ref.py
(itself checked against fp64 autograd, with the sensitivity of the checker used here, by tests/test_dgrad_ref.py).

Families: csrc/conv.hip conv_igemm at both pipeline depths (the gather form), csrc/conv_lds.hip LDS and LDS-DMA in
both rings (the sub-pixel phase plan of make_plan) with K splits 1, 2, 4 and 8, csrc/conv_patch.hip patch and
persistent patch (the transposed halo).  Every launch reads dy from a NaN-poisoned buffer (every column and gap
outside the slice), writes dx into a buffer holding the sentinel everywhere (guard rows, foreign columns, group
gaps), and is run twice.  tests/test_bwd_join_gpu.py covers the epilogue's fused statistics; this file the geometry.

Assertions on every launch of an integer case: dx bit-equal to bf16_rne(reference), dx finite, every sentinel
outside the slice intact, the split-K tickets back at zero, the second run() bit-equal to the first (into a
re-poisoned buffer).  The two real-valued cases: |err| <= 2^-8 |ref| + K 2^-24 T on every element (one bf16 ulp
plus the worst case of an fp32 accumulation of K = KH KW Co + sources addends, T = dgrad(|dy|, |w|) +
sum|sources|) -- derived, not measured.

Minimum configs per family (``min_ran``, from the constraints in csrc/conv_lds.hip make_plan and csrc/conv_patch.hip
patch_plan): every implicit-GEMM config takes every model geometry here: igemm 14, igemm_deep 14, lds 60 (8 tiles x
KC 64 / 128 without the 128 x 128 tile at KC 128, x 4 splits), glds 56 (8 tiles + the 6 with a deep ring, x 4
splits).  The patch kernels take 3x3 / stride 1 with the dy channels Co a multiple of the staged slice cb: Co = 48
gives the 5 tiles x cb 16, Co = 32 the 5 tiles x cb 16, 32; the persistent form holds one slice (Co == cb): 5 at
Co = 32.  (family, case) pairs whose minimum is zero are not generated.

The strides no model uses, (2, 1) and 3: conv_igemm's gather form takes any stride; make_plan takes at most 4
sub-pixel phases, so (2, 1) runs and 3 (9 phases) is refused with -2 (ValueError from prepare); the patch kernels
refuse both.  Each config refuses at prepare time or is exact; the test prints which.

Worst observed values on MI355X (printed by every test, ``Checker.done``; docs/ACCURACY.md "Data gradient"): 0
mismatching elements, written sentinels, non-finite outputs or non-zero tickets in every integer case, config and
second run; randn err / bound 0.977 (3x3 s2) and 0.811 (1x7) in every family.  One host bug found: make_plan wrote
the nine phase records of a stride-3 request into the plan's four before counting them; it now refuses first.
"""
import pytest
import torch

import dgrad_ref as D
from test_bwd_join_gpu import FAMILIES, GEMM_FAMILIES, _families

pytestmark = pytest.mark.gpu

SPLITS = (1, 2, 4, 8)
EXPECT = {"igemm": 14, "igemm_deep": 14, "lds": 60, "glds": 56}


@pytest.fixture(scope="module")
def fn():
    from mtl_das_pytorch_amd.ops import functional as fn
    return fn


def families(fn):
    """test_bwd_join_gpu._families with every K split of the LDS-staged kernels."""
    f = dict(_families(fn))
    f["lds"] = [fn.lds_cfg(t, kc, sp) for t in range(8) for kc in (64, 128) if not (kc == 128 and t == 3)
                for sp in SPLITS]
    f["glds"] = [fn.glds_cfg(t, sp, deep) for deep in (False, True) for t in (fn.GDEEP_TILES if deep else range(8))
                 for sp in SPLITS]
    return f


PATCH_CB = (16, 32, 64)   # functional.PATCH_CB (asserted below): known without the extension, to build the parameters
PATCH_NTILES = 5


def min_ran(family, c):
    """Configs of ``family`` that must accept case ``c`` (see the module docstring)."""
    if family in GEMM_FAMILIES:
        return EXPECT[family]
    if (c.KH, c.KW, c.sh, c.sw) != (3, 3, 1, 1):
        return 0
    cbs = [cb for cb in PATCH_CB if c.Co % cb == 0]
    if family == "patch_persistent":
        cbs = [cb for cb in cbs if cb == c.Co]
    return PATCH_NTILES * len(cbs)


def pairs(cases):
    return [(f, c.name) for c in cases for f in FAMILIES if min_ran(f, c) > 0]


def test_minimum_config_counts(fn):
    assert tuple(fn.PATCH_CB) == PATCH_CB and len(fn.PATCH_TILES) == PATCH_NTILES
    assert {f: len(families(fn)[f]) for f in GEMM_FAMILIES} == EXPECT
    assert [min_ran(f, D.DCASES["3x3 p1"]) for f in FAMILIES] == [14, 14, 60, 56, 5, 0]
    assert [min_ran(f, D.DCASES["3x3 p0"]) for f in FAMILIES] == [14, 14, 60, 56, 10, 5]
    # every family sees the pitched dy, the dx slice, the groups with gaps, cin_stored and the map below a tile
    for name in ("pitched dy", "dx slice", "G3 gaps", "cin8 Ci1", "cin8 Ci3", "B1 1x6", "3x3 p0"):
        assert all(min_ran(f, D.DCASES[name]) > 0 for f in FAMILIES), name


# ---------------------------------------------------------------------------------------------------
class Problem:
    """Device copies of one case's inputs and its reference (computed once per module)."""

    def __init__(self, c):
        self.c = c
        inp = D.dgrad_inputs(c)
        ref = D.dgrad(c, inp)
        if c.real:
            ref["bound"] = D.randn_bound(c, ref)
        self.dybuf, self.w = inp["dybuf"].cuda(), inp["w"].cuda()
        self.srcs = [s.cuda() for s in inp["srcs"]]
        self.out0 = D.dx_buf(c).cuda()
        self.dref = {k: v.cuda() for k, v in ref.items()}


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(D.DCASES[name])
    return _problems[name]


def launch(fn, P, cfg):
    """One launch of problem ``P`` into a fresh sentinel-filled dx buffer: (flat buffer, prepared call), or None when
    the config refuses the geometry at prepare time."""
    c = P.c
    flat = P.out0.clone()
    out, dy = D.dx_view(flat, c), D.dy_view(P.dybuf, c)
    one = c.G == 1   # the ungrouped form of the API

    def sq(t):
        return t[0] if one else t
    try:
        call = fn.prepare_conv2d_dgrad(sq(dy), sq(P.w), (c.H, c.W), (c.sh, c.sw), (c.ph, c.pw),
                                       cin_stored=c.Cs if c.Cs != c.Ci else None, cfg=cfg,
                                       groups=None if one else c.G, add=[sq(s) for s in P.srcs] or None, out=sq(out))
    except ValueError:
        return None
    call.run()
    return flat, call


def check(chk, what, P, flat, call):
    """Every assertion on one launch (module docstring), the second run() included."""
    c = P.c
    if c.real:
        chk.dgrad_bounded(what, c, flat, P.dref)
        chk.true(what + " finite", bool(torch.isfinite(D.dx_view(flat, c).float()).all()))
    else:
        chk.dgrad_exact(what, c, flat, P.dref)
    tickets = call._ws[1] if call._ws else None
    if tickets is not None:
        chk.true(what + " split-K tickets", int(tickets.abs().sum()) == 0)
    first = flat.clone()
    flat.copy_(P.out0)
    call.run()
    chk.bits(what + " second run", flat, first)
    if tickets is not None:
        chk.true(what + " split-K tickets (second run)", int(tickets.abs().sum()) == 0)


def sweep(fn, family, name):
    """Every config of ``family`` on case ``name``: (checker, configs that ran, configs that refused)."""
    P, chk, ran, refused = problem(name), D.Checker(), [], []
    for cfg in families(fn)[family]:
        res = launch(fn, P, cfg)
        if res is None:
            refused.append(cfg)
            continue
        ran.append(cfg)
        check(chk, f"cfg {cfg}", P, *res)
    return chk, ran, refused


@pytest.mark.parametrize("family,name", pairs(D.ICASES))
def test_dgrad_exact(fn, family, name):
    chk, ran, _ = sweep(fn, family, name)
    chk.done()
    need = min_ran(family, D.DCASES[name])
    assert len(ran) >= need, (len(ran), need)


@pytest.mark.parametrize("family,name", pairs(D.RCASES))
def test_dgrad_randn(fn, family, name):
    chk, ran, _ = sweep(fn, family, name)
    chk.done()
    need = min_ran(family, D.DCASES[name])
    assert len(ran) >= need, (len(ran), need)


@pytest.mark.parametrize("name", [c.name for c in D.UCASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_dgrad_unused_strides(fn, family, name):
    """Strides (2, 1) and 3: every config refuses the shape at prepare time or is exact."""
    chk, ran, refused = sweep(fn, family, name)
    print(f"{family} {name}: exact {ran} refused {refused}")
    chk.done()
    assert len(ran) + len(refused) == len(families(fn)[family])
    # which it did is fixed by the plans (module docstring): the gather form takes any stride, make_plan at most
    # four phases, the patch kernels stride 1 only
    takes = family.startswith("igemm") or (family in GEMM_FAMILIES and name == "3x3 s(2,1)")
    assert (not refused) if takes else (not ran), (ran, refused)


@pytest.mark.parametrize("family,name", [(f, n) for f, n in pairs([D.DCASES[n] for n in D.XCD_CASES])])
def test_dgrad_xcd_order(fn, family, name):
    """The CONV_XCD tile order over the (multi-phase) grid: the first and the last config of the family that take
    the case, exact and bitwise equal to the plain order."""
    P, chk = problem(name), D.Checker()
    cfgs = [cfg for cfg in families(fn)[family] if launch(fn, P, cfg) is not None]
    assert cfgs
    for cfg in sorted({cfgs[0], cfgs[-1]}):
        plain, xcd = launch(fn, P, cfg), launch(fn, P, cfg | fn.CONV_XCD)
        chk.bits(f"cfg {cfg} xcd == plain", xcd[0], plain[0])
        check(chk, f"cfg {cfg} xcd", P, *xcd)
    chk.done()
