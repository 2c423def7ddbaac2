"""CPU checks of tests/fwd_ref.py: the fp64 references against fp64 torch (F.conv2d, F.batch_norm, nn.BatchNorm2d,
F.max_pool2d), the exactness conditions of the integer inputs of tests/test_fwd_path_gpu.py, and the sensitivity of
every checker that file uses (a reference perturbed the way a subtly wrong kernel would be is rejected, with the
offending element named -- no kernel is mutated)."""
import pytest
import torch
import torch.nn.functional as F

import bwd_ref
import fwd_ref as R
from wpath_ref import NAN, SENT

INT_CASES = [c for c in R.FCASES if not c.real]


@pytest.fixture(scope="module")
def base():
    c = R.FCASE["3x3 p1"]
    inp = R.conv_inputs(c)
    return c, inp, R.conv_fwd(c, inp)


# ---------------------------------------------------------------------------------------------------
# the references against torch
@pytest.mark.parametrize("c", R.FCASES + R.RCASES, ids=lambda c: c.name)
def test_conv_fwd_matches_torch(c):
    """conv_fwd equals fp64 F.conv2d on the concatenated segments as the buffers hold them."""
    inp = R.conv_inputs(c)
    ref = R.conv_fwd(c, inp)
    segs = [R.in_view(inp["buf0"], c)] + ([R.in_view(inp["buf1"], c, 1)] if c.C1 else [])
    x = torch.cat(segs, -1).double()
    assert not torch.isnan(x).any() and torch.equal(x, inp["x"])
    for z in range(c.G):
        y = F.conv2d(x[z].permute(0, 3, 1, 2), inp["w"][z].double(), None if inp["b"] is None else inp["b"][z].double(),
                     (c.sh, c.sw), (c.ph, c.pw)).permute(0, 2, 3, 1)
        if c.real:
            assert torch.allclose(ref["y"][z], y, rtol=1e-12, atol=1e-12)
        else:
            assert torch.equal(ref["y"][z], y)
        assert torch.allclose(ref["s1"][z], y.sum((0, 1, 2)), rtol=1e-12, atol=1e-9)
        assert torch.allclose(ref["s2"][z], (y * y).sum((0, 1, 2)), rtol=1e-12)
    assert ref["ybf"].dtype == torch.bfloat16 and tuple(ref["y"].shape) == (c.G, c.B, c.Ho, c.Wo, c.Co)
    # every element of the buffers outside the slices is NaN, every element of the output buffer the sentinel
    for seg, buf in enumerate([inp["buf0"]] + ([inp["buf1"]] if c.C1 else [])):
        nread = R.in_view(buf, c, seg).numel()
        assert int(torch.isnan(buf.float()).sum()) == buf.numel() - nread
    flat = R.out_buf(c)
    assert R.out_foreign(flat, c).numel() == flat.numel() - c.G * c.M * c.Co and bool((flat.float() == SENT).all())


def test_cases_address_their_buffers():
    """Slices inside their pitches, every base and stride a multiple of 8 channels (16-byte loads), M a multiple of
    no tile height, Co = 48 a partial tile in every width."""
    for c in R.FCASES + R.RCASES + R.NCASES:
        assert c.off0 + c.C0 <= c.ld0 and c.ooff + c.Co <= c.ldo and (not c.C1 or c.off1 + c.C1 <= c.ld1), c.name
        assert not any(v % 8 for v in (c.C0, c.C1, c.Co, c.ld0, c.ld1, c.ldo, c.off0, c.off1, c.ooff, c.gap, c.ogap)), c.name
        assert (c.B, c.H, c.W) in (R.BASE, R.DEEP)
        assert all(c.M % bm for bm in (32, 64, 128, 256) if c.M > bm), c.name   # (3x3 p0: 1200 = 75 x 16)
        if c.M in (1428, 378):
            assert all(c.M % bm for bm in (16, 32, 64, 128, 256) if c.M > bm), c.name
    assert len(R.FCASE) == len(R.FCASES + R.RCASES + R.NCASES)  # the GPU file caches its problems by name


def _bn_case(C=12, G=2, shape=(2, 5, 7)):
    d = R.tail_y(1, shape, C, G)
    return d, shape[0] * shape[1] * shape[2]


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_bn_consts_and_tails_match_torch(eps):
    d, n = _bn_case()
    k, var = R.bn_consts(R.totals(d["y"]), n, d["gamma"], d["beta"], eps)
    k2, _ = R.bn_consts(R.totals(d["y2"]), n, d["gamma2"], d["beta2"], eps)
    for z in range(2):
        def bn(y, sfx):
            return F.batch_norm(y[z].double().permute(0, 3, 1, 2), None, None, d["gamma" + sfx][z].double(),
                                d["beta" + sfx][z].double(), True, 0.1, eps).permute(0, 2, 3, 1)
        t, t2, r = bn(d["y"], ""), bn(d["y2"], "2"), d["r"][z].double()
        assert torch.allclose(var[z], d["y"][z].double().var((0, 1, 2), unbiased=False), rtol=1e-10)
        assert torch.allclose(k[z, 2], d["y"][z].double().mean((0, 1, 2)), rtol=1e-12, atol=1e-14)
        want = {R.ACT_NONE: t, R.ACT_RELU: t.relu(), R.ACT_SIGMOID: t.sigmoid(), R.SIGMUL: t.sigmoid() * r,
                R.ADD_RELU: (t + r).relu(),
                R.POOL_RELU: F.max_pool2d(t.relu().permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)}
        for kind, w in want.items():
            got = R.tail_fwd(kind, d["y"][z], k[z], d["r"][z])
            assert got.shape == w.shape and torch.allclose(got, w, rtol=1e-9, atol=1e-10), kind
        got = R.tail_fwd(R.ADD_RELU, d["y"][z], k[z], d["y2"][z], k2[z])
        assert torch.allclose(got, (t + t2).relu(), rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("shape", [(2, 17, 42), (2, 9, 21), (1, 1, 6)], ids=str)
def test_pool_is_ceil_mode(shape):
    t = torch.randn(shape + (8,), dtype=torch.float64, generator=None)
    want = F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert torch.equal(R.pool2x2_ceil(t), want)
    assert want.shape[1:3] == ((shape[1] + 1) // 2, (shape[2] + 1) // 2)


@pytest.mark.parametrize("momentum,eps", [(0.1, 1e-5), (0.25, 1e-3)])
def test_running_matches_batchnorm(momentum, eps):
    """What nn.BatchNorm2d in train mode leaves in its buffers, in fp64, from non-trivial start values."""
    d, n = _bn_case()
    k, var = R.bn_consts(R.totals(d["y"]), n, d["gamma"], d["beta"], eps)
    for z in range(2):
        m = torch.nn.BatchNorm2d(d["y"].shape[-1], eps=eps, momentum=momentum).double()
        with torch.no_grad():
            m.running_mean.copy_(d["rm"][z])
            m.running_var.copy_(d["rv"][z])
        m.train()
        m(d["y"][z].double().permute(0, 3, 1, 2))
        rm, rv = R.running(d["rm"][z], d["rv"][z], k[z, 2], var[z], n, momentum)
        assert torch.allclose(rm, m.running_mean, rtol=1e-12, atol=1e-14)
        assert torch.allclose(rv, m.running_var, rtol=1e-12, atol=1e-14)
        assert int(m.num_batches_tracked) == 1
    # count == 1 keeps the biased variance
    _, rv = R.running(d["rm"][0], d["rv"][0], k[0, 2], var[0], 1, momentum)
    assert torch.equal(rv, (1 - momentum) * d["rv"][0].double() + momentum * var[0])


def test_eval_consts():
    d, _ = _bn_case()
    k = R.eval_consts(d["rm"], d["rv"], d["gamma"], d["beta"], 1e-3)
    y = d["y"][0].double()
    want = F.batch_norm(y.permute(0, 3, 1, 2), d["rm"][0].double(), d["rv"][0].double(), d["gamma"][0].double(),
                        d["beta"][0].double(), False, 0.1, 1e-3).permute(0, 2, 3, 1)
    assert torch.allclose(R.tail_fwd(R.ACT_NONE, y, k[0]), want, rtol=1e-10, atol=1e-12)


def test_spread_sums_to_totals():
    tot = R.totals(R.tail_y(2, (2, 3, 4), 8, 2)["y"])
    for nrep in (1, 4, 32):
        rep = R.spread(tot, nrep, 32, 5, fill=1e30)
        assert torch.allclose(rep[:, :nrep].sum(1), tot, rtol=1e-14) and bool((rep[:, nrep:] == 1e30).all())
        assert nrep == 1 or not torch.equal(rep[:, 0], rep[:, 1])


# ---------------------------------------------------------------------------------------------------
# exactness conditions
@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: c.name)
def test_integer_cases_stay_exact(c):
    """Per channel sum|y| < 2^24 and sum(y^2) < 2^24 (so is every partial sum, in any order); the inputs are
    bf16-exact integers."""
    inp = R.conv_inputs(c)
    ref = R.conv_fwd(c, inp)
    for t in (inp["x"], inp["w"].double()) + ((inp["b"].double(),) if c.bias else ()):
        assert torch.equal(t, t.round()) and torch.equal(t.float().bfloat16().double(), t)
    assert float(inp["x"].abs().max()) == 4 and float(inp["w"].abs().max()) == c.wlim
    assert 0.3 < float((inp["w"] == 0).float().mean()) < 0.7
    assert float(ref["y"].abs().sum((1, 2, 3)).max()) < 2 ** 24
    assert float(ref["s2"].max()) < 2 ** 24
    assert float(ref["T"].max()) < 2 ** 24 and torch.equal(ref["y"], ref["y"].round())


def test_some_integer_output_needs_rounding():
    """|y| > 256 occurs (odd values there are not bf16 numbers), so the stored y and the unrounded y differ and
    sum(y^2) tells which one the statistics were taken from."""
    c = R.FCASE["3x3 s2"]
    ref = R.conv_fwd(c, R.conv_inputs(c))
    assert not torch.equal(ref["ybf"].double(), ref["y"])


@pytest.mark.parametrize("c", R.NCASES, ids=lambda c: c.name)
def test_nol_ambiguous_share(c):
    d = R.nol_inputs(c, big_shift="big shift" in c.name)
    n = c.B * c.H * c.W
    k, _ = R.bn_consts(R.totals(d["y"]), n, d["gamma"], d["beta"], 1e-5)
    k = k.float().double()
    for kind in (R.ACT_NONE, R.ACT_RELU):
        for z in range(c.G):
            a, amb = R.nol_operand(d["y"][z], k[z, 0], k[z, 1], kind)
            assert float(amb.double().mean()) <= 0.01
            assert torch.equal(a.float().bfloat16().double(), a)
            v = d["y"][z].double() * k[z, 0] + k[z, 1]
            if kind == R.ACT_RELU:
                v = v.clamp_min(0)
            assert bool(((a - v).abs() <= 0.5 * R.ulp_bf16(v)).all())
    if "big shift" in c.name:
        assert float(k[:, 1].abs().min()) > 1.0


def test_nol_ambiguity_map():
    """An operand exactly on a rounding boundary, one a hair off it and one well inside."""
    y = torch.tensor([1.00390625, 1.00390625 * (1 + 2.0 ** -22), 1.001, -1.00390625, 0.0], dtype=torch.float64)
    one, zero = torch.ones(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    a, amb = R.nol_operand(y, one, zero, R.ACT_NONE)
    assert amb.tolist() == [True, True, False, True, False]
    assert float(R.ulp_bf16(torch.tensor(1.0))) == 2.0 ** -7 and float(R.ulp_bf16(torch.tensor(0.75))) == 2.0 ** -8


def test_tail_inputs_off_the_relu_decisions():
    """No ACT_RELU / POOL_RELU / ADD_RELU argument of the real-valued tail inputs lies within bwd_ref.JOIN_MARGIN of
    zero (bwd_ref.mask decides the same elements)."""
    assert R.TAIL_MARGIN == bwd_ref.JOIN_MARGIN
    for seed, shape, C, G in [(48, R.BASE, 48, 1), (8, R.BASE, 8, 1), (60, R.DEEP, 48, 2), (70, (1, 1, 6), 48, 1)]:
        d = R.tail_y(seed, shape, C, G)
        assert not bool(R.relu_arguments_close(d, R.TAIL_MARGIN).any())
        k, k2 = R.tail_consts(d)
        for z in range(G):
            for kind, r, kk2 in ((bwd_ref.ACT_RELU, None, None), (bwd_ref.ADD_RELU, d["r"][z], None),
                                 (bwd_ref.ADD_RELU, d["y2"][z], k2[z])):
                _, amb = bwd_ref.mask(kind, d["y"][z], k[z], r, kk2, ambig=bwd_ref.JOIN_MARGIN)
                assert not bool(amb.any())


# ---------------------------------------------------------------------------------------------------
# sensitivity: every checker of the GPU file rejects the reference of a subtly wrong kernel at a named element
def _flat_of(c, y):
    flat = R.out_buf(c)
    R.out_view(flat, c).copy_(y)
    return flat


def _stats_of(c, s1, s2, nrep=32):
    st = torch.zeros(c.G, 32, 2, c.Co, dtype=torch.float64)
    st[:, 0, 0], st[:, nrep - 1, 1] = s1, s2
    return st


def _rejected(chk, kind):
    assert chk.bad, "the wrong reference passed"
    assert any(b[1] == kind and "first at" in b[2] for b in chk.bad), chk.bad
    return chk.bad


def test_checker_accepts_the_reference(base):
    c, inp, ref = base
    chk = R.Checker()
    assert chk.conv_exact("ref", c, _flat_of(c, ref["ybf"]), _stats_of(c, ref["s1"], ref["s2"], 4), ref, nrep=4)
    chk.done()


def test_rejects_dropped_border_tap(base):
    c, inp, ref = base
    y = R.conv2d_nhwc(inp["x"][0], inp["w"][0], inp["b"][0], c, skip=(0, 1, c.Ho - 1))  # bottom border row, one tap
    y[:-1] = ref["y"][0][:-1]                                                            # ... of the last image only
    y[-1, :, :c.Wo - 6] = ref["y"][0][-1, :, :c.Wo - 6]                                  # ... of one tile's tail
    assert 0 < int((y != ref["y"][0]).sum()) <= 6 * c.Co
    chk = R.Checker()
    assert not chk.conv_exact("tap", c, _flat_of(c, y.float().bfloat16()[None]), None, ref)
    bad = _rejected(chk, "exact")
    assert "(0, 1, 16," in bad[0][2]   # group 0, image 1, output row 16


def test_rejects_one_pixel_missing_from_sum(base):
    c, inp, ref = base
    px = ref["y"][0, 1, 7, 13]
    assert float(px[5]) != 0
    s1 = ref["s1"].clone()
    s1[0, 5] -= px[5]
    chk = R.Checker()
    assert not chk.stat_totals("pixel", _stats_of(c, s1, ref["s2"]), ref)
    assert "(0, 5)" in _rejected(chk, "exact")[0][2]


def test_rejects_sum_of_squares_of_rounded_y():
    c = R.FCASE["3x3 s2"]
    ref = R.conv_fwd(c, R.conv_inputs(c))
    yb = ref["ybf"].double()
    chk = R.Checker()
    assert not chk.stat_totals("rounded", _stats_of(c, ref["s1"], (yb * yb).sum((1, 2, 3))), ref)
    _rejected(chk, "exact")


def test_rejects_bias_added_twice(base):
    c, inp, ref = base
    y = ref["y"] + inp["b"].double()[:, None, None, None]      # every K split added the bias
    chk = R.Checker()
    assert not chk.conv_exact("bias", c, _flat_of(c, y.float().bfloat16()), None, ref)
    _rejected(chk, "exact")
    chk = R.Checker()
    assert not chk.stat_totals("bias", _stats_of(c, y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))), ref)


def test_rejects_padding_fed_as_shift():
    c = R.FCASE["nol big shift"]
    d = R.nol_inputs(c, big_shift=True)
    k, _ = R.bn_consts(R.totals(d["y"]), c.B * c.H * c.W, d["gamma"], d["beta"], 1e-5)
    k = k.float().double()
    for kind in (R.ACT_NONE, R.ACT_RELU):
        a, amb = R.nol_operand(d["y"][0], k[0, 0], k[0, 1], kind)
        ref, extra = R.nol_conv(a, amb, d["w"][0], c)
        pad = k[0, 1].clamp_min(0) if kind == R.ACT_RELU else k[0, 1]
        wrong = R.conv2d_nhwc(a, d["w"][0], None, c, pad_value=pad.float().bfloat16().double())
        assert torch.equal(wrong[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1])   # only the border pixels see the padding
        chk = R.Checker()
        assert chk.act("ref", ref.float().bfloat16(), ref, extra)
        assert not chk.act("pad", wrong.float().bfloat16(), ref, extra)
        _rejected(chk, "act")


def _running_case():
    d, n = _bn_case(C=16, G=1)
    k, var = R.bn_consts(R.totals(d["y"]), n, d["gamma"], d["beta"], 1e-5)
    return d, n, k, var


def test_rejects_biased_variance_and_swapped_momentum():
    d, n, k, var = _running_case()
    m = 0.25
    rm, rv = R.running(d["rm"], d["rv"], k[:, 2], var, n, R.f32(m))
    chk = R.Checker()
    assert chk.running_stats("ref", rm.float(), rv.float(), d["rm"], d["rv"], k[:, 2], var, n, m)
    _, rv_b = R.running(d["rm"], d["rv"], k[:, 2], var, 1, R.f32(m))          # biased variance
    assert not chk.running_stats("biased", rm.float(), rv_b.float(), d["rm"], d["rv"], k[:, 2], var, n, m)
    assert _rejected(chk, "run_var")[0][0] == "biased"
    chk = R.Checker()
    rm_w, rv_w = R.running(d["rm"], d["rv"], k[:, 2], var, n, 1 - R.f32(m))   # momentum on the old value
    assert not chk.running_stats("swapped", rm_w.float(), rv_w.float(), d["rm"], d["rv"], k[:, 2], var, n, m)
    _rejected(chk, "run_mean")


def test_rejects_replicas_read_with_pitch_c(base):
    """A C = 32 BN at channel offset 16 of replica rows 48 wide, read with pitch 32 instead of sld = 48."""
    c, inp, ref = base
    C, coff, sld = 32, 16, c.Co
    st = R.spread(torch.stack([ref["s1"], ref["s2"]], 1), 4, 32, 3)[0]          # [NREP, 2, 48]
    g = R.gen(4)
    gamma, beta = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    flat = st.reshape(-1)[coff:]

    def totals(pitch):
        idx = torch.arange(C)
        return torch.stack([sum(flat[r * 2 * pitch + idx] for r in range(4)),
                            sum(flat[r * 2 * pitch + pitch + idx] for r in range(4))])
    good, _ = R.bn_consts(totals(sld), c.M, gamma, beta, 1e-5)
    want, _ = R.bn_consts(torch.stack([ref["s1"][0, coff:coff + C], ref["s2"][0, coff:coff + C]]), c.M, gamma, beta, 1e-5)
    chk = R.Checker()
    assert chk.consts("sld", good.float(), want, beta)
    wrong, _ = R.bn_consts(totals(C), c.M, gamma, beta, 1e-5)
    assert not chk.consts("pitch C", wrong.float().nan_to_num(0.0), want, beta)
    _rejected(chk, "mean")


def test_rejects_floor_mode_pooling():
    d = R.tail_y(70, R.BASE, 48)
    k, _ = R.tail_consts(d)
    ref = R.tail_fwd(R.POOL_RELU, d["y"][0], k[0])
    assert ref.shape[1:3] == (9, 21)
    chk = R.Checker()
    assert chk.act("ref", ref.float().bfloat16(), ref)
    got = ref.float().bfloat16()
    got[:, -1] = SENT                      # H = 17: a floor-mode kernel never writes the last row of windows
    assert not chk.act("floor", got, ref)
    assert "(0, 8, 0, 0)" in _rejected(chk, "act")[0][2]
    full = R.tail_fwd(R.POOL_RELU, d["y"][0, :, :16], k[0])   # ... or fills it from full windows only
    assert full.shape[1] == 8


def test_rejects_write_past_the_output_slice():
    c = R.FCASE["out slice"]
    ref = R.conv_fwd(c, R.conv_inputs(c))
    flat = _flat_of(c, ref["ybf"])
    chk = R.Checker()
    assert chk.conv_exact("ref", c, flat, None, ref)
    body = flat[R.GUARD_ROWS * c.ldo:].view(-1, c.ldo)
    body[100, c.ooff + c.Co] = 1.0          # one column past the slice
    assert not chk.conv_exact("past", c, flat, None, ref)
    _rejected(chk, "sentinel")
    flat = _flat_of(c, ref["ybf"])
    flat[R.GUARD_ROWS * c.ldo - 1] = 0.0    # the last element of the leading guard rows
    chk = R.Checker()
    assert not chk.conv_exact("guard", c, flat, None, ref)
    flat = _flat_of(c, torch.full_like(ref["ybf"], NAN))
    chk = R.Checker()
    assert not chk.conv_exact("nan", c, flat, None, ref)   # a poisoned column was read
