"""CPU: the pool references of tests/pool_ref.py against torch's own pools and their autograd in fp64, on the case list
the GPU suite (tests/test_pools_gpu.py) runs, and the two claims that suite's equalities rest on:

  * integer data: an fp32 evaluation in the kernels' order (sum over sources and window positions, x fp32(1/9) for the
    average, one round-to-nearest-even) is bit-equal to bf16_rne of the fp64 reference for every committed case;
  * real data: the same evaluation stays within one bf16 ulp of the reference and equals its nearest bf16 wherever the
    reference is farther than k 2^-23 sum|terms| from a rounding boundary.  That margin alone would exclude 1-12 % of
    a case's elements (sums of bf16 values tie exactly in 1-3 % of them, and 54 zero-mean terms cancel), so elements
    whose fp32 sum is exact in any order are held to the rounding of the exact arithmetic instead
    (pool_ref.check_real); what is left with the one-ulp bound alone is at most 0.5 % of every case.

The tie, NaN and -inf rules of the max pool are compared with torch here, not assumed.
"""
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R
from fwd_ref import bf16_rne
from wpath_ref import Checker

MAPS = [("max", hw) for hw in R.MAX_MAPS] + [("avg", hw) for hw in R.AVG_MAPS]
IDS = [f"{k}{h}x{w}" for k, (h, w) in MAPS]


def _same(a, b):
    """Equal element by element, a NaN only matching a NaN."""
    return bool((torch.isnan(a) == torch.isnan(b)).all() and (a[~torch.isnan(a)] == b[~torch.isnan(b)]).all())


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("kind,hw", MAPS, ids=IDS)
def test_reference_is_torchs_pool(kind, hw):
    for c in R.cases(kind, hw):
        inp = R.inputs(c)
        ref = R.reference(c, inp)
        x = _nchw(inp["x"].double()).requires_grad_(True)
        go = _nchw(torch.stack(inp["g"]).double().sum(0))
        if c.is_max:
            y, idx = F.max_pool2d(x, 3, 2, return_indices=True)
            Ho, Wo = c.out_hw
            ih, iw = idx // c.W, idx % c.W
            oh = torch.arange(Ho).view(1, 1, Ho, 1)
            ow = torch.arange(Wo).view(1, 1, 1, Wo)
            am = (ih - 2 * oh) * 3 + (iw - 2 * ow)
            assert torch.equal(_nhwc(am), ref["am"]), c.name
            assert _same(_nhwc(y.detach()), ref["y"]), c.name
        else:
            y = F.avg_pool2d(x, 3, 1, 1)
            assert torch.allclose(_nhwc(y.detach()), ref["y"], rtol=0, atol=1e-13), c.name
        y.backward(go)
        dx = _nhwc(x.grad)
        assert not torch.isnan(dx).any()
        if not c.is_max:  # torch spreads g / 9 term by term, the reference divides the sum
            assert torch.allclose(dx, ref["dx"], rtol=0, atol=1e-12), c.name
        elif c.real:      # the order of a pixel's (at most 4) windows
            assert torch.allclose(dx, ref["dx"], rtol=0, atol=1e-13), c.name
        else:
            assert torch.equal(dx, ref["dx"]), c.name
        if c.is_max:
            assert (ref["dx"][:, R.uncovered(c.H, c.W)] == 0).all()


def test_max_pool_rules_in_isolation():
    """One window each: first maximum, a NaN wins, the last NaN gives the position, -inf stays at position 0."""
    inf = float("inf")
    rows = {"tie": ([1, 3, 3, 0, 3, -1, 2, 3, 1], 3.0, 1), "nan wins": ([1, 9, R.NAN, 0, 10, 0, 0, 0, 0], R.NAN, 2),
            "last nan": ([R.NAN, 0, 0, 0, R.NAN, 0, 5, 0, 0], R.NAN, 4), "-inf": ([-inf] * 9, -inf, 0),
            "zeros": ([-0.0, 0.0, 0, 0, 0, 0, 0, 0, 0], 0.0, 0)}
    for name, (vals, want, pos) in rows.items():
        x = torch.tensor(vals, dtype=torch.float64).view(1, 3, 3, 1)
        y, am = R.max_fwd(x)
        ty, ti = F.max_pool2d(_nchw(x), 3, 2, return_indices=True)
        assert _same(y.view(-1), torch.tensor([want], dtype=torch.float64)) and int(am) == pos, name
        assert _same(ty.view(-1), y.view(-1)) and int(ti) == pos, name


def _emulate(c, inp, ref):
    """The kernels' arithmetic in fp32 on the CPU: (y, dx of the stored-argmax / average kernel, dx of the window
    re-reading max kernel or None), each rounded once to bf16."""
    x = inp["x"]
    ninth = torch.tensor(1.0 / 9.0, dtype=torch.float32)
    Ho, Wo = c.out_hw
    if c.is_max:
        y = ref["y"].float()  # a maximum is one of its inputs
        am = ref["am"]
        dx1 = torch.zeros(c.B, c.H, c.W, c.C)
        for g in inp["g"]:            # per source, the covering windows in (oh, ow) order: window position descending
            for t in reversed(range(9)):
                R._win(dx1, t // 3, t % 3, Ho, Wo).add_(torch.where(am == t, g, torch.zeros_like(g)))
        gs = torch.zeros_like(inp["g"][0])
        for g in inp["g"]:            # the re-reading kernel sums the sources of one window first
            gs = gs + g
        dx2 = torch.zeros(c.B, c.H, c.W, c.C)
        for t in reversed(range(9)):
            R._win(dx2, t // 3, t % 3, Ho, Wo).add_(torch.where(am == t, gs, torch.zeros_like(gs)))
        return y.bfloat16(), dx1.bfloat16(), dx2.bfloat16()

    def sum9(acc, t):
        p = torch.zeros(c.B, c.H + 2, c.W + 2, c.C)
        p[:, 1:c.H + 1, 1:c.W + 1] = t
        for k in range(9):
            acc = acc + p[:, k // 3:k // 3 + c.H, k % 3:k % 3 + c.W]
        return acc
    y = sum9(torch.zeros(c.B, c.H, c.W, c.C), x) * ninth
    acc = torch.zeros(c.B, c.H, c.W, c.C)
    for g in inp["g"]:
        acc = sum9(acc, g)
    return y.bfloat16(), (acc * ninth).bfloat16(), None


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("kind,hw", MAPS, ids=IDS)
def test_fp32_evaluation_meets_the_gpu_suites_equalities(kind, hw):
    chk, worst, n_int = Checker(), 0.0, 0
    for c in R.cases(kind, hw):
        inp = R.inputs(c)
        ref = R.reference(c, inp)
        y, dx1, dx2 = _emulate(c, inp, ref)
        if not c.real:
            if not c.is_max:  # (the maximum of a NaN / -inf window is compared by test_reference_is_torchs_pool)
                chk.bits(c.name + " y", y, bf16_rne(ref["y"]).float().bfloat16())
            chk.bits(c.name + " dx", dx1, bf16_rne(ref["dx"]).float().bfloat16())
            if dx2 is not None:
                chk.exact(c.name + " dx is exact in bf16", dx1, ref["dx"])
                chk.bits(c.name + " dx (re-read)", dx2, dx1)
            n_int += dx1.numel()
            continue
        shares = [R.check_real(chk, c, "dx", dx1, ref)]
        if c.is_max:
            shares.append(R.check_real(chk, c, "dx", dx2, ref))
        else:
            shares.append(R.check_real(chk, c, "y", y, ref))
        worst = max(worst, max(shares))
        assert max(shares) <= R.EXCLUDED_CAP, (c.name, shares)
    print(f"{kind} {hw[0]}x{hw[1]}: {n_int} integer-case gradient elements bit-equal; worst excluded near-boundary "
          f"share of a real case {worst:.4%} (cap {R.EXCLUDED_CAP:.2%})")
    chk.done()


def test_boundary_distance():
    """1 + 2^-8 is the midpoint of the bf16 neighbours 1 and 1 + 2^-7; below 1 the step halves."""
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 - 2.0 ** -9 - 2.0 ** -20, 1.0, 3.0, -1.0 - 2.0 ** -8],
                     dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -20, 2.0 ** -20, 2.0 ** -9, 2.0 ** -7, 0.0], dtype=torch.float64)
    assert torch.allclose(R.boundary_distance(v), want, rtol=0, atol=1e-15)


def test_sliced_layout():
    v = torch.arange(12.0).view(2, 2, 3)
    buf = R.sliced(v, 8, 2, R.SENT)
    own, rest = R.owned(buf, 2, 3)
    assert buf.shape == (4, 8) and torch.equal(own, v.view(4, 3)) and (rest == R.SENT).all() and rest.numel() == 20


def test_grid_stride_cases_take_a_second_trip():
    for name, (is_max, backward, B, H, W, C) in R.GRID_CASES.items():
        Ho, Wo = R.max_out_hw(H, W) if is_max else (H, W)
        items = B * (H * W if backward else Ho * Wo) * C // 8
        assert R.GRID_ITEMS < items < 2 ** 31, (name, items)
