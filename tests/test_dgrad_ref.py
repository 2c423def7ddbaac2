"""CPU checks of tests/dgrad_ref.py: the scatter reference against fp64 autograd of F.conv2d and against
bwd_ref.join, the exactness conditions of the integer inputs of tests/test_dgrad_gpu.py, and the sensitivity of the
checker that file uses (the output a subtly wrong kernel would leave is rejected, with the offending element named
-- no kernel is mutated); last, the return codes of the host plan for strides no model uses (parsed, never
launched)."""
import pytest
import torch
import torch.nn.functional as F

import bwd_ref
import dgrad_ref as D
from wpath_ref import SENT

ALL = D.ICASES + D.UCASES + D.RCASES
INT_CASES = D.ICASES + D.UCASES


def _ref(name):
    c = D.DCASES[name]
    inp = D.dgrad_inputs(c)
    return c, inp, D.dgrad(c, inp)


# ---------------------------------------------------------------------------------------------------
# the reference against torch
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_scatter_matches_autograd_and_join(c):
    inp = D.dgrad_inputs(c)
    ref = D.dgrad(c, inp)
    dyv = D.dy_view(inp["dybuf"], c).double()
    assert not torch.isnan(dyv).any() and torch.equal(dyv, inp["dy"])
    assert int(torch.isnan(inp["dybuf"].float()).sum()) == inp["dybuf"].numel() - dyv.numel()
    assert tuple(ref["dx"].shape) == (c.G, c.B, c.H, c.W, c.Cs) and ref["dxbf"].dtype == torch.bfloat16
    for z in range(c.G):
        x = torch.zeros(c.B, c.Ci, c.H, c.W, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, inp["w"][z].double(), None, (c.sh, c.sw), (c.ph, c.pw))
        assert tuple(y.shape[2:]) == (c.Ho, c.Wo)
        y.backward(inp["dy"][z].permute(0, 3, 1, 2))
        srcs = [s[z] for s in inp["srcs"]]
        want = x.grad.permute(0, 2, 3, 1) + sum(s[..., :c.Ci].double() for s in srcs)
        join = bwd_ref.join(inp["w"][z], inp["dy"][z].bfloat16(), (c.H, c.W), (c.sh, c.sw), (c.ph, c.pw),
                            [s[..., :c.Ci] for s in srcs])
        got = ref["dx"][z, ..., :c.Ci]
        if c.real:
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12) and torch.allclose(got, join, rtol=1e-12, atol=1e-12)
        else:
            assert torch.equal(got, want) and torch.equal(got, join)
        # the stored channels without a weight receive the sources only
        assert torch.equal(ref["dx"][z, ..., c.Ci:], sum(s[..., c.Ci:].double() for s in srcs) + torch.zeros(c.B, c.H, c.W, c.Cs - c.Ci))
    flat = D.dx_buf(c)
    assert D.dx_foreign(flat, c).numel() == flat.numel() - c.G * c.M * c.Cs and bool((flat.float() == SENT).all())


def test_cases_address_their_buffers():
    """Slices inside their pitches, every base and stride a multiple of 8 channels (16-byte loads); the names are
    unique (the GPU file caches its problems by name); the geometry each case is there for."""
    assert len(D.DCASES) == len(ALL)
    for c in ALL:
        assert c.doff + c.Co <= c.ldd and c.ooff + c.Cs <= c.ldo and c.Ci <= c.Cs, c.name
        assert not any(v % 8 for v in (c.Co, c.Cs, c.ldd, c.ldo, c.doff, c.ooff, c.dgap, c.ogap)), c.name
    left = D.DCASES["3x3 s2 p0 leftover"]
    assert (left.Ho, left.Wo) == (3, 5) and (left.Ho - 1) * 2 + 3 == left.H - 1 and (left.Wo - 1) * 2 + 3 == left.W - 1
    fit = D.DCASES["3x3 s2 p0 fit"]
    assert (fit.Ho - 1) * 2 + 3 == fit.H and (fit.Wo - 1) * 2 + 3 == fit.W
    assert D.DCASES["3x3 s2 one row"].H == 1 and D.DCASES["3x3 s2 odd"].H % 2 and D.DCASES["3x3 s2 odd"].W % 2
    assert D.DCASES["1x1 s2"].Co * 1 <= 64                       # one K chunk of 64 under 8 splits
    assert all((c.KH * c.KW * c.Co) % 32 for c in (D.DCASES["3x3 p1 Co40"], D.DCASES["3x3 p1 Co8"]))
    assert all(D.DCASES["3x3 p1"].M % bm for bm in (16, 32, 64, 128, 256))
    assert D.DCASES["B1 1x6"].M < 16


@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: c.name)
def test_integer_cases_stay_exact(c):
    """T = dgrad(|dy|, |w|) + sum|sources| bounds every partial sum of an element in any order: below 2^24 the fp32
    accumulator holds each exactly."""
    inp = D.dgrad_inputs(c)
    ref = D.dgrad(c, inp)
    assert float(ref["T"].max()) < 2.0 ** 24
    for t in [inp["dy"], inp["w"]] + inp["srcs"]:
        assert torch.equal(t.double(), t.double().round()) and torch.equal(t.bfloat16().double(), t.double())
    assert float(inp["dy"].abs().max()) == 4 and float(inp["w"].abs().max()) == c.wlim
    assert float(ref["dx"].abs().max()) > 0


def test_some_integer_output_needs_rounding():
    """|dx| beyond 256 is no longer a bf16 integer: the bit comparison sees the kernel's rounding mode."""
    c, inp, ref = _ref("1x7")
    assert bool((ref["dxbf"].double() != ref["dx"]).any())


def test_leftover_is_zero_or_the_source():
    c, inp, ref = _ref("3x3 s2 p0 leftover")
    assert bool((ref["dx"][:, :, 7] == 0).all()) and bool((ref["dx"][:, :, :, 11] == 0).all())
    c, inp, ref = _ref("3x3 s2 p0 leftover src")
    s = inp["srcs"][0].double()
    assert torch.equal(ref["dx"][:, :, 7], s[:, :, 7]) and torch.equal(ref["dx"][:, :, :, 11], s[:, :, :, 11])
    assert bool((s[:, :, 7] != 0).any())


# ---------------------------------------------------------------------------------------------------
# sensitivity: the GPU file's checker rejects what a subtly wrong kernel would leave, at a named element
def _flat_of(c, dx):
    flat = D.dx_buf(c)
    D.dx_view(flat, c).copy_(dx)
    return flat


def _rejected(chk, kind, at=None):
    assert chk.bad, "the wrong output passed"
    hit = [b for b in chk.bad if b[1] == kind and "first at" in b[2]]
    assert hit, chk.bad
    if at is not None:
        assert f"first at {at}" in hit[0][2], hit[0][2]
    return hit


def _first_diff(a, b):
    ne = a.double() != b.double()
    i = int(ne.reshape(-1).int().argmax())
    return tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ne.shape))


def _wrong(c, inp, **kw):
    dx = torch.stack([D.scatter(kw.pop("dy", inp["dy"])[z], kw.pop("w", inp["w"])[z], c, **kw) for z in range(c.G)])
    for s in inp["srcs"]:
        dx = dx + s.double()
    return dx


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_checker_accepts_the_reference(c):
    inp = D.dgrad_inputs(c)
    ref = D.dgrad(c, inp)
    chk = D.Checker()
    assert chk.dgrad_exact("ref", c, _flat_of(c, ref["dxbf"]), ref)
    ref["bound"] = D.randn_bound(c, ref)
    assert chk.dgrad_bounded("ref", c, _flat_of(c, ref["dxbf"]), ref)
    chk.done()


@pytest.mark.parametrize("name", ["3x3 s2 p0 leftover", "3x3 s2 p0 leftover src"])
def test_rejects_unwritten_leftover(name):
    """The leftover row / column of a valid stride-2 conv left as it was (sentinel) instead of 0 (+ source)."""
    c, inp, ref = _ref(name)
    for sl, at in (((slice(None), slice(None), 7), (0, 0, 7, 0, 0)), ((slice(None), slice(None), slice(None), 11), (0, 0, 0, 11, 0))):
        got = ref["dxbf"].clone()
        got[sl] = SENT
        chk = D.Checker()
        assert not chk.dgrad_exact("leftover", c, _flat_of(c, got), ref)
        _rejected(chk, "exact", at)


def test_rejects_dropped_border_tap_of_one_phase():
    """Tap (1, 0) missing from the bottom row of dx in the odd columns only: one sub-pixel phase, one border."""
    c, inp, ref = _ref("3x3 s2 odd")
    ih = c.H - 1                                   # row 16 = 2 * 8 - 1 + kh: reached by kh = 1 from oh = 8
    assert (ih + c.ph - 1) % c.sh == 0
    wrong = _wrong(c, inp, drop=(1, 0, ih, 1))     # tap (1, 0) lands on the odd columns iw = 2 ow - 1
    assert torch.equal(wrong[:, :, :ih], ref["dx"][:, :, :ih]) and torch.equal(wrong[..., 0::2, :], ref["dx"][..., 0::2, :])
    at = _first_diff(R_bf(wrong), ref["dxbf"])
    assert at[:4] == (0, 0, ih, 1)
    chk = D.Checker()
    assert not chk.dgrad_exact("tap", c, _flat_of(c, R_bf(wrong)), ref)
    _rejected(chk, "exact", at)


def R_bf(dx):
    return D.R.bf16_rne(dx).float().bfloat16()


def test_rejects_phase_residue_without_padding():
    """rh = py % sh instead of (py + ph) % sh: each phase reduces over the taps of the padding-0 conv."""
    c, inp, ref = _ref("3x3 s2 odd")
    wrong = _wrong(c, inp, pad=(0, 0))
    chk = D.Checker()
    assert not chk.dgrad_exact("residue", c, _flat_of(c, R_bf(wrong)), ref)
    _rejected(chk, "exact", _first_diff(R_bf(wrong), ref["dxbf"]))


@pytest.mark.parametrize("name", ["3x3 p1", "1x7", "5x5 p2"])
def test_rejects_mirrored_taps(name):
    c, inp, ref = _ref(name)
    wrong = _wrong(c, inp, w=inp["w"].flip(3, 4))
    chk = D.Checker()
    assert not chk.dgrad_exact("mirror", c, _flat_of(c, R_bf(wrong)), ref)
    _rejected(chk, "exact", _first_diff(R_bf(wrong), ref["dxbf"]))


def test_rejects_source_added_once_per_split():
    c, inp, ref = _ref("1x1 s2 src")
    wrong = ref["dx"] + inp["srcs"][0].double()    # two K splits, each adding the source
    at = _first_diff(R_bf(wrong), ref["dxbf"])
    chk = D.Checker()
    assert not chk.dgrad_exact("source", c, _flat_of(c, R_bf(wrong)), ref)
    _rejected(chk, "exact", at)
    # an empty phase's pixel (odd row): the reference there is the source alone
    assert torch.equal(ref["dx"][:, :, 1], inp["srcs"][0].double()[:, :, 1])


def test_rejects_nonzero_padding_channels():
    c, inp, ref = _ref("cin8 Ci1")
    got = ref["dxbf"].clone()
    got[0, 1, 4, 7, c.Ci] = 1.0
    chk = D.Checker()
    assert not chk.dgrad_exact("channels", c, _flat_of(c, got), ref)
    _rejected(chk, "exact", (0, 1, 4, 7, c.Ci))


@pytest.mark.parametrize("name", ["pitched dy", "G3 gaps"])
def test_rejects_dy_read_with_pitch_co(name):
    """dy read as rows of Co instead of ldd elements: the poisoned columns enter (NaN), or the wrong pixels."""
    c, inp, ref = _ref(name)
    P = c.B * c.Ho * c.Wo
    flatdy = inp["dybuf"].float()[:, c.doff:]
    dense = flatdy[:, :P * c.Co].reshape(c.G, c.B, c.Ho, c.Wo, c.Co).double()
    wrong = _wrong(c, inp, dy=dense)
    chk = D.Checker()
    assert not chk.dgrad_exact("pitch", c, _flat_of(c, wrong.float().bfloat16()), ref)
    assert ("pitch finite", "condition") in chk.bad
    _rejected(chk, "exact")
    # with the poison taken out (a buffer whose other columns hold finite data) the values still differ
    wrong0 = _wrong(c, inp, dy=dense.nan_to_num(1.0))
    chk = D.Checker()
    assert not chk.dgrad_exact("pitch", c, _flat_of(c, R_bf(wrong0)), ref)
    _rejected(chk, "exact", _first_diff(R_bf(wrong0), ref["dxbf"]))


def test_rejects_write_past_the_dx_slice():
    c, inp, ref = _ref("dx slice")
    flat = _flat_of(c, ref["dxbf"])
    chk = D.Checker()
    assert chk.dgrad_exact("ref", c, flat, ref)
    body = flat[D.R.GUARD_ROWS * c.ldo:].view(-1, c.ldo)
    body[100, c.ooff + c.Cs] = 1.0                # one column past the slice
    assert not chk.dgrad_exact("past", c, flat, ref)
    _rejected(chk, "sentinel")
    flat = _flat_of(c, ref["dxbf"])
    flat[D.R.GUARD_ROWS * c.ldo - 1] = 0.0        # the last element of the guard rows before the buffer
    chk = D.Checker()
    assert not chk.dgrad_exact("guard", c, flat, ref)
    _rejected(chk, "sentinel")


def test_rejects_dx_groups_without_the_gap():
    """Group z of dx stored z buffers further instead of z (buffer + gap)."""
    c, inp, ref = _ref("G3 gaps")
    assert c.ogap
    flat = D.dx_buf(c)
    g0 = D.R.GUARD_ROWS * c.ldo
    for z in range(c.G):
        flat[g0 + z * c.M * c.ldo:g0 + (z + 1) * c.M * c.ldo].view(c.B, c.H, c.W, c.ldo)[..., c.ooff:c.ooff + c.Cs] = ref["dxbf"][z]
    chk = D.Checker()
    assert not chk.dgrad_exact("gap", c, flat, ref)
    at = _rejected(chk, "exact")[0][2]
    assert "first at (0, 1, 8, 20," in at or "first at (1," in at   # group 0 is in place; the first wrong element is
    _rejected(chk, "sentinel")                                      # where group 1 begins (or its gap's sentinel)


def test_randn_bound_rejects_one_missing_tap():
    """The per-element bound of the real-valued cases still sees one tap missing at one border row."""
    c, inp, ref = _ref("real 3x3 s2")
    ref["bound"] = D.randn_bound(c, ref)
    wrong = _wrong(c, inp, drop=(1, 0, c.H - 1, 1))
    chk = D.Checker()
    assert not chk.dgrad_bounded("tap", c, _flat_of(c, wrong.float().bfloat16()), ref)
    _rejected(chk, "dx")


# ---------------------------------------------------------------------------------------------------
# host plan (no launch, no GPU): what csrc/conv_lds.hip make_plan does with strides no model uses
@pytest.mark.parametrize("stride,rc", [((1, 1), 0), ((2, 2), 0), ((2, 1), 0), ((4, 1), 0), ((3, 3), -2), ((5, 1), -2)])
def test_plan_refuses_more_than_four_phases(stride, rc):
    """A data gradient has sh * sw sub-pixel phases and the plan record holds four: beyond that every LDS-staged
    config answers -2 (the plan used to fill nine phase records of stride 3 before it counted them)."""
    from mtl_das_pytorch_amd.ops import functional as fn
    from mtl_das_pytorch_amd.ops.hip import lib
    c = D.DCase("plan", 2, 10, 22, 32, 32, sh=stride[0], sw=stride[1])
    d = {"src": {"p0": 4096, "ld0": c.Co, "C0": c.Co, "C1": 0, "gs0": 0}, "w": 4096, "wgs": 0, "out": 4096,
         "ldo": c.Cs, "ogs": 0, "B": c.B, "Hs": c.Ho, "Ws": c.Wo, "Ho": c.H, "Wo": c.W, "N": c.Cs, "Npad": 32,
         "Cs": c.Co, "KH": 3, "KW": 3, "sh": c.sh, "sw": c.sw, "ph": 1, "pw": 1, "Kpad": 288}   # parsed, never launched
    for cfg in (fn.lds_cfg(0), fn.lds_cfg(1, 128, 8), fn.glds_cfg(0, 4), fn.glds_cfg(0, 2, True)):
        assert lib().conv_workspace(1, cfg, 1, d)[0] == rc, cfg
