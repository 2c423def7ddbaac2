"""The Inception pools at kernel level (csrc/misc.hip pool3_fwd_kernel<0 / 1>, pool3_bwd_kernel<0 / 1 / 2>) against
the fp64 references of tests/pool_ref.py (themselves checked against torch on the CPU by tests/test_pool_ref.py).  The
binding is called directly, in the forms the engine launches: x, y and dx channel slices of wider buffers, up to 6
gradient sources each with its own pitch and channel offset (one of them all zeros), the stored-argmax backward from
the kernel's own argmax and from the reference's, the window re-reading backward.

Maps: max 3x3, 4x7, 5x6, 8x9, 7x3 (even H / W: the last row / column is in no window); average 1x9, 9x1, 2x2, 3x5, 6x7;
B 1 and 3; C 8, 24 (slice 8.. of 40), 72 (slice 16.. of 96); 1, 2, 6 sources.  On the 8x9 map: a NaN four windows
cover, two NaNs in one window, a -inf window, a constant 6x6 patch.  One launch per instantiation with more work
items than one trip of the 4096 x 256 grid (data and fp64 reference on the device).

Equalities (none derived from what the kernels give; tests/test_pool_ref.py shows on the CPU that an fp32 evaluation
in the kernels' order meets each of them on these very cases):
  integer data  every stored value is bit-equal to bf16_rne(reference): maxima and argmax bytes, both max-pool
                gradients (bit-equal to each other too), the average and its gradient.
  real data     a maximum is one of its inputs: bit-equal.  Sums: within one bf16 ulp (fwd_ref.one_ulp) everywhere and
                the nearest bf16 wherever pool_ref.check_real can tell which one that is; the share of a case's
                elements left with the ulp bound alone is at most 0.5 %.
  foreign       the other channels of the y / dx buffers, the guard tail of every buffer and the argmax bytes past
                B Ho Wo C are bit-unchanged.
  poison        NaN in the other channels of x and of every source and, for the max pool, in the pixels no window
                covers: a result that read one of them is NaN and fails its equality; dx there is exactly +0.
"""
import pytest
import torch

import pool_ref as R
from fwd_ref import bf16_rne
from wpath_ref import Checker

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel elements after every buffer


def _lib():
    from mtl_das_pytorch_amd.ops.hip import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def P(t, off=0):
    return t.data_ptr() + off * t.element_size()


def _bf16_buffer(buf2d):
    """A [M][ld] fp32 CPU buffer as flat device bf16 followed by GUARD sentinels."""
    flat = torch.full((buf2d.numel() + GUARD,), R.SENT, dtype=torch.bfloat16)
    flat[:buf2d.numel()] = buf2d.reshape(-1).bfloat16()
    return flat.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bits_nan(chk, what, got, ref):
    """bf16 ``got`` against fp64 ``ref`` whose values are exact in bf16: NaN where the reference is NaN, the same bits
    everywhere else (-inf and the sign of a zero included)."""
    want = ref.float().bfloat16()
    gn, rn = torch.isnan(got), torch.isnan(want)
    chk.true(what + ": NaN exactly where the reference is", torch.equal(gn, rn))
    chk.exact(what, _bits(got)[~rn], _bits(want)[~rn])


def _rne(ref):
    return bf16_rne(ref).float().bfloat16()


class Launch:
    """The device buffers of one PCase and its launches."""

    def __init__(self, c, chk):
        self.c, self.chk = c, chk
        self.inp = R.inputs(c)
        self.ref = R.reference(c, self.inp)
        self.Ho, self.Wo = c.out_hw
        self.Mi, self.Mo = c.B * c.H * c.W, c.B * self.Ho * self.Wo
        self.x = _bf16_buffer(R.sliced(self.inp["x"], c.ld, c.off, R.NAN))
        self.g = [_bf16_buffer(R.sliced(g, ld, off, R.NAN)) for g, (ld, off) in zip(self.inp["g"], c.srcs)]
        self.shares = []

    def geom(self):
        c = self.c
        return {"x": P(self.x, c.off), "ldx": c.ld, "B": c.B, "H": c.H, "W": c.W, "C": c.C, "Ho": self.Ho, "Wo": self.Wo}

    def _foreign(self, what, flat, M):
        c = self.c
        own, rest = R.owned(flat[:M * c.ld].view(M, c.ld), c.off, c.C)
        self.chk.true(f"{c.name} {what}: other channels and the guard tail untouched",
                      bool((rest == R.SENT).all() and (flat[M * c.ld:] == R.SENT).all()))
        return own.cpu()

    def forward(self):
        """Returns the device argmax buffer (max pool)."""
        c, chk = self.c, self.chk
        y = torch.full((self.Mo * c.ld + GUARD,), R.SENT, dtype=torch.bfloat16, device="cuda")
        d = dict(self.geom(), y=P(y, c.off), ldy=c.ld)
        am = None
        if c.is_max:
            am = torch.full((self.Mo * c.C + GUARD,), 255, dtype=torch.uint8, device="cuda")
            d["am"] = P(am)
        _lib().pool3(int(c.is_max), 0, _stream(), d)
        own = self._foreign("y", y, self.Mo).view(c.B, self.Ho, self.Wo, c.C)
        if c.is_max:
            _bits_nan(chk, c.name + " y", own, self.ref["y"])
            a = am.cpu()
            chk.true(c.name + " argmax: bytes past the output still 255", bool((a[self.Mo * c.C:] == 255).all()))
            chk.true(c.name + " argmax: every owned byte <= 8", int(a[:self.Mo * c.C].max()) <= 8)
            chk.exact(c.name + " argmax", a[:self.Mo * c.C].view(c.B, self.Ho, self.Wo, c.C), self.ref["am"])
        elif c.real:
            self.shares.append(R.check_real(chk, c, "y", own, self.ref))
        else:
            chk.bits(c.name + " y", own, _rne(self.ref["y"]))
        return am

    def backward(self, what, am=None):
        """One backward launch; returns the owned dx (CPU bf16)."""
        c, chk = self.c, self.chk
        dx = torch.full((self.Mi * c.ld + GUARD,), R.SENT, dtype=torch.bfloat16, device="cuda")
        d = dict(self.geom(), dx=P(dx, c.off), lddx=c.ld,
                 g=[(P(g, off), 0, ld) for g, (ld, off) in zip(self.g, c.srcs)])
        if am is not None:
            d["am"] = P(am)
        _lib().pool3(int(c.is_max), 1, _stream(), d)
        own = self._foreign("dx " + what, dx, self.Mi).view(c.B, c.H, c.W, c.C)
        if c.real:
            self.shares.append(R.check_real(chk, c, "dx", own, self.ref))
        else:
            chk.bits(f"{c.name} dx {what}", own, _rne(self.ref["dx"]))
        if c.is_max:
            chk.true(f"{c.name} dx {what}: +0 where no window covers",
                     bool((_bits(own[:, R.uncovered(c.H, c.W)]) == 0).all()))
        return own

    def run(self):
        c, chk = self.c, self.chk
        am = self.forward()
        if c.is_max:
            ref_am = torch.full((self.Mo * c.C + GUARD,), 255, dtype=torch.uint8)
            ref_am[:self.Mo * c.C] = self.ref["am"].reshape(-1).to(torch.uint8)
            a = self.backward("(kernel's argmax)", am)
            b = self.backward("(reference's argmax)", ref_am.cuda())
            r = self.backward("(windows re-read)")
            chk.bits(c.name + " dx: the two argmax sources agree", a, b)
            if not c.real:
                chk.bits(c.name + " dx: stored argmax and re-read windows agree", a, r)
        else:
            self.backward("")
        for s in self.shares:
            chk._note("share of elements with the ulp bound alone", s)
            chk.true(f"{c.name}: {s:.4%} of the elements left with the ulp bound alone (cap {R.EXCLUDED_CAP:.2%})",
                     s <= R.EXCLUDED_CAP)


MAPS = [("max", hw) for hw in R.MAX_MAPS] + [("avg", hw) for hw in R.AVG_MAPS]


@pytest.mark.parametrize("kind,hw", MAPS, ids=[f"{k}{h}x{w}" for k, (h, w) in MAPS])
def test_pool_against_fp64(kind, hw):
    chk = Checker()
    cs = R.cases(kind, hw)
    for c in cs:
        Launch(c, chk).run()
    torch.cuda.synchronize()
    print(f"{kind} {hw[0]}x{hw[1]}: {len(cs)} cases")
    chk.done()


# ---------------------------------------------------------------------------------------------------
# more work items than one trip of the grid
def _dev_ints(g, shape):
    v = torch.randint(-4, 5, shape, generator=g, device="cuda").float()
    return v * (torch.rand(shape, generator=g, device="cuda") >= 0.16)


def _guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


@pytest.mark.parametrize("name", list(R.GRID_CASES))
def test_grid_stride_second_trip(name):
    """Integer data generated on the device, the reference in fp64 on the device (the only cases that compute one
    there), contiguous buffers, two gradient sources: bit-equal."""
    is_max, backward, B, H, W, C = R.GRID_CASES[name]
    reread = "re-read" in name
    Ho, Wo = R.max_out_hw(H, W) if is_max else (H, W)
    items = B * (H * W if backward else Ho * Wo) * C // 8
    assert items > R.GRID_ITEMS
    chk = Checker()
    g = torch.Generator(device="cuda").manual_seed(77)
    x32 = _dev_ints(g, (B, H, W, C))
    x = _guarded(x32.numel(), torch.bfloat16, R.SENT)
    x[:x32.numel()] = x32.reshape(-1).bfloat16()
    d = {"x": P(x), "ldx": C, "B": B, "H": H, "W": W, "C": C, "Ho": Ho, "Wo": Wo}
    n_out = B * Ho * Wo * C
    if not backward:
        y = _guarded(n_out, torch.bfloat16, R.SENT)
        d.update(y=P(y), ldy=C)
        am = None
        if is_max:
            am = _guarded(n_out, torch.uint8, 255)
            d["am"] = P(am)
        _lib().pool3(is_max, 0, _stream(), d)
        got = y[:n_out].view(B, Ho, Wo, C)
        if is_max:
            ry, ram = R.max_fwd(x32.double())
            chk.exact(name + " y", got, ry)
            chk.exact(name + " argmax", am[:n_out].view(B, Ho, Wo, C), ram)
            chk.true("argmax guard", bool((am[n_out:] == 255).all()))
        else:
            chk.bits(name + " y", got, _rne(R.avg_fwd(x32.double())))
        chk.true("y guard", bool((y[n_out:] == R.SENT).all()))
    else:
        gs32 = [_dev_ints(g, (B, Ho, Wo, C)) for _ in range(2)]
        gs = []
        for t in gs32:
            b = _guarded(n_out, torch.bfloat16, R.SENT)
            b[:n_out] = t.reshape(-1).bfloat16()
            gs.append(b)
        dx = _guarded(x32.numel(), torch.bfloat16, R.SENT)
        d.update(dx=P(dx), lddx=C, g=[(P(b), 0, C) for b in gs])
        gsum = gs32[0].double() + gs32[1].double()
        if is_max:
            _, ram = R.max_fwd(x32.double())
            ref = R.max_bwd(gsum, ram, H, W)
            if not reread:
                am = _guarded(n_out, torch.uint8, 255)
                am[:n_out] = ram.reshape(-1).to(torch.uint8)
                d["am"] = P(am)
        else:
            ref = R.avg_bwd(gsum)
        _lib().pool3(is_max, 1, _stream(), d)
        chk.bits(name + " dx", dx[:x32.numel()].view(B, H, W, C), _rne(ref))
        chk.true("dx guard", bool((dx[x32.numel():] == R.SENT).all()))
    print(f"{name}: {items} work items, {items / R.GRID_ITEMS:.2f} trips of the grid")
    chk.done()


# ---------------------------------------------------------------------------------------------------
# what the binding and the launcher refuse (csrc/bindings.cpp pool3, csrc/misc.hip launch_pool3): every check below is
# host code that throws before the launch
def _d(*dicts, **kw):
    """The dicts merged left to right, then the keywords."""
    out = {}
    for d in dicts:
        out.update(d)
    out.update(kw)
    return out


def test_pool3_refuses_malformed_arguments():
    B, H, W, C, ld = 2, 5, 6, 8, 16
    Ho, Wo = R.max_out_hw(H, W)
    x = torch.zeros(B * H * W * ld + GUARD, dtype=torch.bfloat16, device="cuda")
    y = _guarded(B * H * W * ld, torch.bfloat16, R.SENT)       # large enough for the average's output too
    dx = _guarded(B * H * W * ld, torch.bfloat16, R.SENT)
    g = torch.zeros(B * H * W * ld + GUARD, dtype=torch.bfloat16, device="cuda")
    am = _guarded(B * H * W * C, torch.uint8, 255)
    geo_max = {"x": P(x), "ldx": ld, "B": B, "H": H, "W": W, "C": C, "Ho": Ho, "Wo": Wo}
    geo_avg = _d(geo_max, Ho=H, Wo=W)
    fwd = {"y": P(y), "ldy": ld}
    bwd = {"dx": P(dx), "lddx": ld, "g": [(P(g), 0, ld), (P(g, 8), 0, ld)]}
    one = {"dx": P(dx), "lddx": ld, "g": P(g), "ldg": ld}     # the single-pointer form
    bad = [
        # forward
        (1, 0, _d(geo_max, fwd, ldx=12), "ldx"), (1, 0, _d(geo_max, fwd, ldx=0), "ldx"),
        (1, 0, _d(geo_max, fwd, ldy=4), "ldy"), (0, 0, _d(geo_avg, fwd, ldy=20), "ldy"),
        (1, 0, _d(geo_max, fwd, x=P(x) + 2), "x must be 16-byte"), (1, 0, _d(geo_max, fwd, y=P(y) + 8), "y must be 16-byte"),
        (1, 0, _d(geo_max, fwd, am=P(am) + 4), "am must be 8-byte"),
        (1, 0, _d(geo_max, fwd, x=0), "x is null"), (0, 0, _d(geo_avg, ldy=ld), "y is null"),
        (1, 0, _d(geo_max, fwd, B=0), "positive"), (1, 0, _d(geo_max, fwd, H=0), "positive"),
        (0, 0, _d(geo_avg, fwd, W=-1), "positive"), (1, 0, _d(geo_max, fwd, C=0), "positive"),
        (1, 0, _d(geo_max, fwd, C=12), "C % 8"),
        (1, 0, _d(geo_max, fwd, Ho=Ho + 1), "Ho, Wo"), (1, 0, _d(geo_max, fwd, Wo=Wo - 1), "Ho, Wo"),
        (1, 0, _d(geo_max, fwd, H=2, Ho=0), "3 x 3"), (0, 0, _d(geo_avg, fwd, Ho=H - 1), "Ho, Wo"),
        (0, 0, _d(geo_avg, fwd, am=P(am)), "argmax only for max"),
        # backward
        (1, 1, _d(geo_max, bwd, lddx=12), "lddx"), (0, 1, _d(geo_avg, bwd, lddx=0), "lddx"),
        (1, 1, _d(geo_max, bwd, dx=0), "dx is null"), (0, 1, _d(geo_avg, bwd, dx=P(dx) + 4), "dx must be 16-byte"),
        (1, 1, _d(geo_max, bwd, g=[]), "no gradient source"), (0, 1, _d(geo_avg, dx=P(dx), lddx=ld), "no gradient source"),
        (0, 1, _d(geo_avg, one, g=0), "null gradient source"), (1, 1, _d(geo_max, bwd, g=[(0, 0, ld)]), "null gradient source"),
        (0, 1, _d(geo_avg, one, g=P(g) + 2), "g must be 16-byte"), (0, 1, _d(geo_avg, one, ldg=4), "ldg"),
        (0, 1, _d(geo_avg, one, ldg=20), "ldg"),
        (1, 1, _d(geo_max, bwd, g=[(P(g), 0, ld), (P(g), 0, 0)]), "source pitch"),
        (1, 1, _d(geo_max, bwd, g=[(P(g), 0, ld), (P(g), 0, 12)]), "pitch"),
        (1, 1, _d(geo_max, bwd, g=[(P(g) + 2, 0, ld)]), "16-byte"), (1, 1, _d(geo_max, bwd, g=[(P(g), 0, ld)] * 7), "at most 6"),
        (1, 1, _d(geo_max, bwd, x=0), "x is null"), (1, 1, _d(geo_max, bwd, x=P(x) + 2), "x must be 16-byte"),
        (1, 1, _d(geo_max, bwd, ldx=4), "ldx"),
        (1, 1, _d(geo_max, bwd, am=P(am) + 4), "am must be 8-byte"),
        # a wrong Ho / Wo would let the window re-reading backward read past the map
        (1, 1, _d(geo_max, bwd, Ho=Ho + 1), "Ho, Wo"), (1, 1, _d(geo_max, bwd, am=P(am), Wo=Wo + 1), "Ho, Wo"),
        (0, 1, _d(geo_avg, bwd, Wo=W + 1), "Ho, Wo"), (0, 1, _d(geo_avg, bwd, B=0), "positive"),
        # the launcher: 2^31 work items or more (32-bit index math in the kernels)
        (0, 0, _d(geo_avg, fwd, B=1 << 20, H=64, W=64, Ho=64, Wo=64), "rc=-2"),
        (0, 1, _d(geo_avg, bwd, B=1 << 20, H=64, W=64, Ho=64, Wo=64), "rc=-2"),
    ]
    for is_max, backward, d, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            _lib().pool3(is_max, backward, _stream(), d)
    torch.cuda.synchronize()
    assert (y == R.SENT).all() and (dx == R.SENT).all() and (am == 255).all()  # nothing was launched
    # the same arguments unbroken are served
    _lib().pool3(1, 0, _stream(), _d(geo_max, fwd, am=P(am)))
    _lib().pool3(1, 1, _stream(), _d(geo_max, bwd, am=P(am)))
    _lib().pool3(1, 1, _stream(), _d(geo_max, bwd))
    _lib().pool3(0, 0, _stream(), _d(geo_avg, fwd))
    _lib().pool3(0, 1, _stream(), _d(geo_avg, one))
    torch.cuda.synchronize()
    assert not (dx[:B * H * W * ld] == R.SENT).all()
