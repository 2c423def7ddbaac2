"""CPU checks of tests/wpath_ref.py: the fp64 references against fp64 autograd / torch.optim.Adam, the exactness of
the integer inputs of tests/test_wpath_gpu.py, the sensitivity of every checker (a reference perturbed the way a
subtly wrong kernel would be is rejected, with the offending element named -- no kernel is mutated), and the host
table builders."""
import math

import pytest
import torch
import torch.nn.functional as F

import wpath_ref as R

ALL_WCASES = R.WCASES + R.WBATCH_IM2COL + R.WBATCH_PATCH


def _autograd_wgrad(x, dy, c):
    """fp64 autograd of F.conv2d: x [B, H, W, Cs], dy [B, Ho, Wo, Co] -> [Co, Cs, KH, KW]."""
    w = torch.zeros(c.Co, c.Cs, c.KH, c.KW, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=(c.sh, c.sw), padding=(c.ph, c.pw))
    y.backward(dy.permute(0, 3, 1, 2))
    return w.grad


@pytest.mark.parametrize("c", ALL_WCASES, ids=lambda c: c.name)
def test_wgrad_ref_matches_autograd(c):
    inp = R.wgrad_inputs(c)
    for z in range(c.G):
        ref = R.to_nchw(R.wgrad_ref(inp["x"][z], inp["dy"][z], c), c)
        auto = _autograd_wgrad(inp["x"][z], inp["dy"][z], c)
        if c.real:
            assert torch.allclose(ref, auto, rtol=1e-12, atol=1e-12)
        else:
            assert torch.equal(ref, auto)  # integers: exact in any order
    # the buffers hold the operands at their slices and NaN everywhere else
    b0 = inp["buf0"][:, :c.B * c.H * c.W * c.ld0].view(c.G, -1, c.ld0)
    assert int(torch.isnan(b0.float()).sum()) == b0.numel() - c.G * c.B * c.H * c.W * c.C0
    assert not torch.isnan(b0[:, :, c.off0:c.off0 + c.C0].float()).any()


@pytest.mark.parametrize("c", [c for c in ALL_WCASES if not c.real], ids=lambda c: c.name)
def test_integer_inputs_stay_exact(c):
    """Every partial sum is an integer below 2^24; the normalise-on-load operand is the same in fp32 and fp64."""
    inp = R.wgrad_inputs(c)
    assert c.M <= R.MAX_PX
    x, dy = inp["x"], inp["dy"]
    assert torch.equal(x, x.round()) or c.nol is not None
    assert torch.equal(x * 2, (x * 2).round()) and torch.equal(dy, dy.round())
    assert torch.equal(x.float().bfloat16().double(), x) and torch.equal(dy.float().bfloat16().double(), dy)
    for z in range(c.G):
        T = R.wgrad_ref(x[z].abs(), dy[z].abs(), c)
        assert float(T.max()) * 2 < 2 ** 24  # (x 2: operands that are multiples of 1/2)
    if c.nol is not None:
        assert torch.equal(inp["x32"].double().view_as(x), x)
        assert torch.isnan(inp["consts"][:, 2:]).all()


def test_cases_address_their_buffers():
    """Slices inside their pitches, every base and stride a multiple of 8 channels (16-byte loads), no map a whole
    number of chunks (every chunk size ends mid-chunk), the finalize's sums below 2^24."""
    for c in ALL_WCASES:
        assert c.off0 + c.C0 <= c.ld0 and c.doff + c.Co <= c.ldd and (not c.C1 or c.off1 + c.C1 <= c.ld1), c.name
        assert not any(v % 8 for v in (c.C0, c.C1, c.Co, c.ld0, c.ld1, c.ldd, c.off0, c.off1, c.doff, c.gap)), c.name
        assert all(c.M % mch for mch in (32, 64, 128, 256) if c.M > mch), c.name
    assert max(R.FIN_SPLITS) * 64 < 2 ** 24
    names = [c.name for c in ALL_WCASES]
    assert len(set(names)) == len(names)  # the GPU file caches its problems by name


def test_real_cases_stay_small():
    for c in ALL_WCASES:
        if c.real:
            assert c.M <= R.MAX_PX  # the bound 2 n 2^-24 T stays a quarter of one average term T / n
            assert 2 * c.M * 2.0 ** -24 <= 0.25 / c.M


def test_split_pixels_partition():
    c = R.WCASES[0]
    for splits, mps, rows in [(3, 704, 0), (1, 1536, 0), (2, 9, 4), (5, 2, 4)]:
        pix = R.split_pixels(c, splits, mps, rows)
        assert torch.equal(pix.sum(0), torch.ones(c.B, c.Ho, c.Wo, dtype=torch.long))
    (s, m), (s1, m1) = R.forced_plans(1428, 64)
    assert (s, m, s1, m1) == (3, 704, 1, 1472) and 0 < 1428 - (s - 1) * m < 64
    for M in (1428, 378, 396, 1200, 732, 840, 266, 280):
        for MCH in (32, 64, 128, 256):
            if M > MCH:
                (s, m), _ = R.forced_plans(M, MCH)
                assert m % MCH == 0 and 2 <= s <= 8 and 0 < M - (s - 1) * m < MCH


def test_stem_virtual_geometry_is_the_real_convolution():
    """The 1 x KW convolution over the packed taps has the real KH x KW convolution's weight gradient."""
    for KH, KW, s, p, H, W in R.STEMS:
        g = R.gen(KH)
        X = R.ints(g, (3, 1, H, W))
        idx = torch.tensor([2, 0, 1])
        real = R.WCase("real", 3, H, W, 1, 8, KH=KH, KW=KW, sh=s, sw=s, ph=p, pw=p)
        virt = R.WCase("virtual", 3, H, W, 8, 8, KH=1, KW=KW, sh=s, sw=s, ph=0, pw=p)
        virt.Ho, virt.Wo = real.Ho, real.Wo
        dy = R.ints(g, (3, real.Ho, real.Wo, 8)).double()
        packed = R.pack_taps_ref(X, idx, KH, p)
        for b in range(3):  # the packing itself, element by element
            for j in range(8):
                for h in range(H):
                    hh = h - p + j
                    exp = X[idx[b], 0, hh] if (j < KH and 0 <= hh < H) else torch.zeros(W)
                    assert torch.equal(packed[b, h, :, j].float(), exp)
        a = R.to_nchw(R.wgrad_ref(X[idx].permute(0, 2, 3, 1).double(), dy, real), real)      # [Co, 1, KH, KW]
        v = R.to_nchw(R.wgrad_ref(packed.double(), dy, virt), virt)                           # [Co, 8, 1, KW]
        assert torch.equal(v[:, :KH, 0, :], a[:, 0]) and not v[:, KH:].any()
        assert torch.equal(a, _autograd_wgrad(X[idx].permute(0, 2, 3, 1).double(), dy, real))


def test_adam_ref_matches_torch_adam():
    hp = dict(b1=0.9, b2=0.999, eps=1e-8, wd=1e-5)
    p0, g0, m0, v0 = (x.double() for x in R.adam_state(500, 7))
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=R.f32(1e-3), betas=(R.f32(0.9), R.f32(0.999)), eps=R.f32(1e-8),
                           weight_decay=R.f32(1e-5), foreach=False)
    cur = {"p": p0, "m": torch.zeros_like(p0), "v": torch.zeros_like(p0)}
    for t in (1, 2, 3):
        g = g0 * t
        p.grad = g.clone()
        opt.step()
        cur = R.adam_ref(cur["p"], g, cur["m"], cur["v"], t, R.f32(1e-3), **hp)
        assert torch.allclose(cur["p"], p.detach(), rtol=1e-13, atol=0)
        st = opt.state[p]
        assert torch.allclose(cur["m"], st["exp_avg"], rtol=1e-13, atol=0)
        assert torch.allclose(cur["v"], st["exp_avg_sq"], rtol=1e-13, atol=0)
    # the update from the stored moments is the step's own
    r =R.adam_ref(p0, g0, m0, v0, 5, 1e-3, **hp)
    assert torch.allclose(r["p"] - p0, R.adam_update(r["m"], r["v"], 5, 1e-3), rtol=1e-9, atol=1e-18)


# ---------------------------------------------------------------------------------------------------
# sensitivity: what a subtly wrong kernel would give is rejected, with the element named
def _rejects(chk, kind=None):
    assert chk.bad, "the checker accepted a perturbed result"
    msg = chk.bad[0]
    assert "first at" in msg[2], msg
    if kind:
        assert msg[1] == kind or kind in str(msg), msg
    with pytest.raises(AssertionError):
        chk.done()


@pytest.mark.parametrize("c", [c for c in R.WCASES if c.name in ("3x3 p1", "two segments", "G2 nol relu")],
                         ids=lambda c: c.name)
@pytest.mark.parametrize("how", ["dropped pixel", "doubled pixel", "shifted tap"])
def test_wgrad_checker_sensitivity(c, how):
    inp = R.wgrad_inputs(c)
    x, dy = inp["x"][0], inp["dy"][0]
    good = R.wgrad_ref(x, dy, c)
    chk = R.Checker()
    assert chk.exact("unperturbed", good.float(), good) and not chk.bad
    b, h, w = 1, c.Ho // 2, c.Wo - 1
    assert dy[b, h, w].any() and R.wgrad_cols(x, c)[b, :, :, h, w].any()
    if how == "dropped pixel":
        pix = torch.ones(c.B, c.Ho, c.Wo, dtype=torch.bool)
        pix[b, h, w] = False
        bad = R.wgrad_ref(x, dy, c, pix)
    elif how == "doubled pixel":
        d2 = dy.clone()
        d2[b, h, w] *= 2
        bad = R.wgrad_ref(x, d2, c)
    else:
        bad = good.roll(1, dims=1)
    _rejects_exact = R.Checker()
    _rejects_exact.exact(how, bad.float(), good)
    _rejects(_rejects_exact, "exact")


def test_wgrad_real_checker_sensitivity():
    """One pixel dropped from a real-valued case exceeds 2 n 2^-24 T at some element; fp32 rounding does not."""
    c = next(c for c in R.WCASES if c.real)
    inp = R.wgrad_inputs(c)
    x, dy = inp["x"][0], inp["dy"][0]
    good, T = R.wgrad_ref(x, dy, c), R.wgrad_ref(x.abs(), dy.abs(), c)
    chk = R.Checker()
    assert chk.wgrad_real("fp32 rounding of the reference", good.float(), good, T, c.M) and not chk.bad
    pix = torch.ones(c.B, c.Ho, c.Wo, dtype=torch.bool)
    pix[0, 3, 5] = False
    chk.wgrad_real("dropped pixel", R.wgrad_ref(x, dy, c, pix).float(), good, T, c.M)
    _rejects(chk, "wgrad")


def test_finalize_checker_sensitivity():
    for d in R.fin_descs(0)[:4] + R.fin_descs(0)[12:]:
        slab = R.fin_slab(d, 1)
        for mem in d["members"]:
            good = R.fin_ref(slab, d, mem, 0.125)
            assert torch.isfinite(good).all()  # no poison in any result
            chk = R.Checker()
            assert chk.exact("unperturbed", good.float(), good)
            chk.exact("one split left out", R.fin_ref(slab, d, mem, 0.125, skip_split=d["splits"] - 1).float(), good)
            _rejects(chk, "exact")
    d = R.fin_descs(0)[12]  # the centre-tap member reads its own tap only: the next tap is NaN
    assert torch.isnan(R.fin_slab(d, 1)[0, 0, 16, 5 * d["Cs"]])


@pytest.mark.parametrize("t", [1, 10])
def test_adam_checker_sensitivity(t):
    old = dict(zip("pgmv", R.adam_state(4000, 3)))
    hp = dict(wd=1e-5, grad_scale=0.125)

    def as_kernel(r):
        return {k: r[k].float() for k in "pmv"}
    chk = R.Checker()
    assert chk.adam("fp32 rounding of the reference", as_kernel(R.adam_ref(*old.values(), t, 1e-3, **hp)), old, t, 1e-3, **hp)
    for what, got in [("t off by one", R.adam_ref(*old.values(), t + 1, 1e-3, **hp)),
                      ("weight decay decoupled", R.adam_ref(*old.values(), t, 1e-3, decoupled=True, **hp)),
                      ("grad_scale ignored", R.adam_ref(*old.values(), t, 1e-3, wd=1e-5))]:
        chk = R.Checker()
        chk.adam(what, as_kernel(got), old, t, 1e-3, **hp)
        _rejects(chk, "adam")
    assert abs(R.adam_tau(1) - 2.4e-4) < 1e-5 and R.adam_tau(10 ** 4) < 1.2e-6


def test_image_checker_sensitivity():
    n, images = R.opt_layout()
    p = R.adam_state(n, 5)[0]
    for im in images:
        wf, wd = R.image_refs(im, p, torch.zeros(im["Npad"], im["Kpad"]).bfloat16(),
                              torch.zeros(im["Npad_d"], im["Kpad_d"]).bfloat16())
        for img in (wf, wd):
            chk = R.Checker()
            assert chk.bits("unperturbed", img.clone(), img)
            chk.bits("one column shifted", torch.cat([img[:, :1].roll(1, 0), img[:, 1:]], 1), img)
            _rejects(chk, "exact")


def test_image_refs_match_the_pack_layouts():
    from mtl_das_pytorch_amd.ops import functional as fn
    n, images = R.opt_layout()
    p = R.adam_state(n, 5)[0]
    for im in images:
        wf, wd = R.image_refs(im, p, torch.zeros(im["Npad"], im["Kpad"]).bfloat16(),
                              torch.zeros(im["Npad_d"], im["Kpad_d"]).bfloat16())
        if len(im["members"]) == 1:
            Co, kh, kw, _, _, off = im["members"][0]
            w = p[off:off + Co * im["Ci"] * kh * kw].view(Co, im["Ci"], kh, kw)
            assert torch.equal(wf, fn.pack_weight_fwd(w, im["Cs"])) and torch.equal(wd, fn.pack_weight_dgrad(w, im["Cs"]))
        else:  # a fused group is the images of the concatenated weight, a centre-tap 1x1 zero-extended to the kernel
            ws = []
            for Co, kh, kw, n0, t0, off in im["members"]:
                w = p[off:off + Co * im["Ci"] * kh * kw].view(Co, im["Ci"], kh, kw)
                full = torch.zeros(Co, im["Ci"], im["KH"] * im["KW"])
                full[:, :, t0:t0 + kh * kw] = w.reshape(Co, im["Ci"], kh * kw)
                ws.append(full.view(Co, im["Ci"], im["KH"], im["KW"]))
            w = torch.cat(ws)
            assert torch.equal(wf, fn.pack_weight_fwd(w, im["Cs"])) and torch.equal(wd, fn.pack_weight_dgrad(w, im["Cs"]))


# ---------------------------------------------------------------------------------------------------
# host tables
@pytest.mark.parametrize("max_out", [0, 2, 8])
def test_wgfin_table_block_counts(monkeypatch, max_out):
    """build_wgfin_table's blocks are the kernel's mappings: ceil(elems / (256 * FIN_EPT)) in output order,
    ceil(G Co taps Cs * lanes / 256) in slab order."""
    from mtl_das_pytorch_amd.engine import core
    from mtl_das_pytorch_amd.ops.hip import lib
    monkeypatch.setattr(core, "FIN_OUT_MAX_SPLITS", max_out)
    assert lib().FIN_EPT == 2
    descs, want = [], []
    for d in R.fin_descs(0) + R.fin_descs(5):
        for Co, kh, kw, n0, t0 in d["members"]:
            descs.append({"slab": 0, "grad": 0, "ggs": 0, "G": d["G"], "splits": d["splits"], "Npad": d["Npad"],
                          "Kpad": d["Kpad"], "Co": Co, "Ci": d["Ci"], "Cs": d["Cs"], "KH": kh, "KW": kw,
                          "elems": d["G"] * Co * d["Ci"] * kh * kw})
            lanes = core.finalize_lanes(d["splits"])
            if d["splits"] <= max_out:
                want.append(math.ceil(descs[-1]["elems"] / 512))
            else:
                want.append(math.ceil(d["G"] * Co * kh * kw * d["Cs"] * lanes / 256))
    totals = [core.build_wgfin_table(descs[:i], "cpu")[2] for i in range(len(descs) + 1)]
    assert [b - a for a, b in zip(totals, totals[1:])] == want
    assert {core.finalize_lanes(s) for s in R.FIN_SPLITS} == {1, 2, 4, 8, 16}
    # element counts off both block sizes are among the descriptors
    assert any(d["elems"] % 512 and d["elems"] % 256 for d in descs)


def test_optimizer_segments_cover_the_part_c_buffer():
    from mtl_das_pytorch_amd.engine import core
    numel, images = R.opt_layout()
    conv = [{"kind": 3, "off": off, "n": Co * im["Ci"] * kh * kw, "Co": Co, "Ci": im["Ci"], "KH": kh, "KW": kw,
             "Cs": im["Cs"]} for im in images for Co, kh, kw, n0, t0, off in im["members"]]
    segs = core.optimizer_segments(conv, numel)
    cover = torch.zeros(numel, dtype=torch.long)
    for s in segs:
        cover[s["off"]:s["off"] + s["n"]] += 1
    assert torch.equal(cover, torch.ones_like(cover))
    plain = [s["n"] for s in segs if s["kind"] == 0]
    assert plain == R.OPT_PLAIN and {4, 1020, 1024, 1028} <= set(plain) and plain[-1] % 1024
    _, ns, nblocks = core.build_optseg_table(segs, "cpu")
    want = sum(math.ceil(s["n"] / 1024) if s["kind"] == 0 else
               math.ceil(s["Co"] / 8) * math.ceil(s["Ci"] / core.pack_tile_ci(s["KH"] * s["KW"])) for s in segs)
    assert ns == len(segs) and nblocks == want
