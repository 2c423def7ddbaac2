"""The weight path at kernel level against the fp64 references of tests/wpath_ref.py (themselves checked on the CPU
by tests/test_wpath_ref.py): dy and x through the weight-gradient kernels into the split slabs, wgrad_finalize into
the flat fp32 gradient, adam_pack into the masters and the two packed bf16 images, and the packed-tap stem end to
end.  The bindings are called directly with descriptors from the project's own builders (build_wgfin_table,
optimizer_segments, build_optseg_table, finalize_lanes, ConvLayer.wgrad_plan, stem_pack_geom), so the host tables
are under test too.

A. Weight-gradient kernels (csrc/conv.hip wgrad_block / wgrad_big_block / WgPatch::run, csrc/wgrad_lean.hip),
   per-conv and batched (capped persistent grid), in the forms the engine launches: groups with their own strides,
   pitched inputs and dy, two segments, normalise-on-load constants per group, the engine's split plan and two
   forced ones (a last split shorter than a chunk; one split), every geometry family, Co off the tile, partial K
   tiles, Cs = 8.
B. wgrad_finalize in both thread mappings (FIN_OUT_MAX_SPLITS 0 / 2 / 8) at 1-129 splits, 1-49 taps, Ci on both
   sides of 256 / taps, Ci < Cs, groups with a gap, fused members over one slab.
C. adam_pack: plain ranges and conv tiles, fused-member images, every mode of the launch.
D. The packed-tap stem: gather_batch (taps / off, cursor, zero ranges), and the chains gather -> wgrad -> finalize
   and adam_pack(update = 0) -> forward conv against the REAL KH x KW convolution of the unpacked input.

Bounds (none derived from what the kernels give):
  exact         A, B, D on integer data: x, dy integers in [-4, 4] (exact in bf16), normalise-on-load with scales
                0.5 / 1 / 2 and integer shifts, finalize scale 1 or 1/8 -- every partial sum is an integer below 2^24
                (tests/test_wpath_ref.py asserts it), so the fp32 result is the fp64 one in ANY order: torch.equal
                after a cast, per split slab, summed, finalized.  NaN poison sits wherever a result must not read
                (input / dy columns outside the addressed slice, the mean / invstd rows of the constants, slab rows
                >= Co, columns >= taps * Cs, channels Ci <= ci < Cs); a sentinel wherever nothing may be written
                (slab and gradient and image surroundings, a guard tail after every buffer).
  wgrad (real)  |got - ref| <= 2 n 2^-24 T per element, n = B Ho Wo addends, T the fp64 gradient of (|x|, |dy|):
                bf16 x bf16 products are exact in fp32, a sequential fp32 sum of n addends loses at most
                (n - 1) 2^-24 T, the factor 2 covers the MFMA's internal adder.  n <= 1428: the bound is a quarter
                of one average term.
  adam m, v     4 * 2^-24 of the sum of the magnitudes of their two addends (gj = g * grad_scale + wd * p: at most
                two roundings; two products and one sum).  The inputs keep |g grad_scale| >= 16 |wd p| and m, v
                away from zero, so neither sum cancels.
  adam update   p_new - p_old against the fp64 formula evaluated on the kernel's OWN stored m and v (so a moment
                that cancels cannot amplify into the update): relative tau(t) = 4 * 2^-24 (1 / (1 - b1^t) +
                1 / (1 - b2^t)) + 8 * 2^-24 -- the cancellation in 1 - powf(b, t) and eight roundings -- plus
                2^-24 |p| for the final rounding of p.  tau(1) = 2.4e-4, tau(10^4) = 1e-6.
  images        bit-exact bf16 of the masters the kernel itself stored; padding, a centre-tap member's other taps
                and a neighbour member's columns bit-unchanged.
  stem forward  exact on integer data whose outputs fit bf16 (|y| <= 98); randn: |got - ref| <= 2^-8 |ref| +
                1e-5 max|ref| (one bf16 ulp, the dx bound of tests/test_bwd_join_gpu.py).

Configs per family (MIN_RAN asserts the count of (case, config) pairs launched, each under three split plans):
  small 0-7, big 32-35, lean 36-43 and lean-big 44-47 take all 17 cases of wpath_ref.WCASES (136 / 68 / 136 / 68
  pairs); whole-reduction 8-11 the cases whose Kpad their TK divides (Kpad 192: 8 and 10 x 5 cases, 128 / 256: 9 x 5,
  320: 11 x 5 -- 20 pairs); patch 12-19 the 3x3 / s1 cases whose rows fit and whose channels split into the slice
  (12, 13: 8 cases each, 14: 3, 15: 1, 16, 17: 3, 18, 19: 6 -- 38 pairs).  Batched tables: every config of a family
  with the jobs of its pool that it takes (MIN_BATCH: configs with at least four jobs; 9 and 11 take two).

Worst observed values on MI355X (printed by every test, ``Checker.done``):
  A  every integer comparison exact (the file makes 4,388 exact comparisons in all: slabs per split and summed,
     batched slabs bit-identical to the per-conv launch under caps 0 / 3 / 7); real-valued cases err / bound
     1.4e-3 (err = 4 * 2^-24 T: the MFMA sums pairwise and a block sums few chunks, far below the sequential
     worst case).
  B  all 15 (threshold, rotation) launches x 2 scales exact, sentinels around every range intact.
  C  m err / bound 0.34, v 0.46; update err / bound 0.987 (the final rounding of p: half an ulp of a p just above
     1.0 is 2^-24 = the whole absolute term of the bound there -- by construction below it); every image
     bit-exact, state bit-unchanged under update = 0, two launches bit-identical to one.
  D  gather, the wgrad -> finalize chain (24 configs x 2 stems) and the integer forward chain exact; randn forward
     err / bound 0.98 (one bf16 ulp next to a power of two, as the dx figure of tests/test_bwd_join_gpu.py).
  No kernel, binding or host table had to change: the tests found no bug.
"""
import math
import types

import pytest
import torch

import wpath_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel elements after every buffer


@pytest.fixture(scope="module")
def fn():
    from mtl_das_pytorch_amd.ops import functional as fn
    return fn


@pytest.fixture(scope="module")
def core():
    from mtl_das_pytorch_amd.engine import core
    return core


def _lib():
    from mtl_das_pytorch_amd.ops.hip import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """Device buffers with a sentinel guard tail; ``check`` asserts every tail is untouched."""

    def __init__(self):
        self.all = []

    def put(self, t, name="buffer"):
        """A device copy of CPU tensor ``t`` followed by GUARD sentinels."""
        full = torch.full((t.numel() + GUARD,), R.SENT, dtype=t.dtype).cuda()
        full[:t.numel()] = t.reshape(-1).cuda()
        self.all.append((name, full, t.numel()))
        return full[:t.numel()].view(t.shape)

    def fill(self, shape, dtype, value, name="buffer"):
        n = math.prod(shape)
        full = torch.full((n + GUARD,), R.SENT, dtype=dtype, device="cuda")
        full[:n] = value
        self.all.append((name, full, n))
        return full[:n].view(shape)

    def check(self, chk):
        for name, full, n in self.all:
            chk.true(f"guard tail of {name}", bool((full[n:] == R.SENT).all()))


def P(t, off=0):
    return t.data_ptr() + off * t.element_size()


def table(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


# ---------------------------------------------------------------------------------------------------
# A. weight-gradient kernels
FAMILIES = {"small": range(0, 8), "whole": range(8, 12), "patch": range(12, 20), "big": range(32, 36),
            "lean": range(36, 44), "leanbig": range(44, 48)}
# (case, config) pairs of WCASES each family must launch: 17 cases x the family's configs where every config takes
# every case (TK 32 / 64 divide every Kpad; the big and lean tiles may be partial); whole-reduction tiles: Kpad 192
# (5 cases x configs 8, 10), 128 / 256 (5 x config 9), 320 (5 x config 11); patch, from patch_valid's rules on the
# 3x3 / s1 cases: configs 12, 13 take 8 cases, 14: 3, 15: 1, 16, 17: 3, 18, 19: 6
MIN_RAN = {"small": 136, "whole": 20, "patch": 38, "big": 68, "lean": 136, "leanbig": 68}
# configs whose batched table holds at least four jobs (configs 9 and 11 take two jobs of the pool each)
MIN_BATCH = {"small": 8, "whole": 2, "patch": 8, "big": 4, "lean": 8, "leanbig": 4}


class WProblem:
    """Device buffers of one WCase and its fp64 references (computed once, cached per split plan)."""

    def __init__(self, c):
        self.c, self.bufs = c, Bufs()
        inp = R.wgrad_inputs(c)
        self.buf0 = self.bufs.put(inp["buf0"], "x0")
        self.buf1 = self.bufs.put(inp["buf1"], "x1") if c.C1 else None
        self.dybuf = self.bufs.put(inp["dybuf"], "dy")
        self.consts = self.bufs.put(inp["consts"], "consts") if c.nol is not None else None
        self.cols = torch.stack([R.wgrad_cols(inp["x"][z], c) for z in range(c.G)]).cuda()
        self.dy = inp["dy"].cuda()
        self.ref = self._ref(None)                                         # [G, Co, taps, Cs]
        self.T = torch.stack([R.wgrad_from_cols(self.cols[z].abs(), self.dy[z].abs()) for z in range(c.G)]) if c.real else None
        self._split = {}
        self.nbase = len(self.bufs.all)

    def drop_slabs(self):
        self.bufs.all = self.bufs.all[:self.nbase]

    def _ref(self, pix):
        return torch.stack([R.wgrad_from_cols(self.cols[z], self.dy[z], pix) for z in range(self.c.G)])

    def split_ref(self, splits, mps, R_rows):
        key = (splits, mps, R_rows)
        if key not in self._split:
            pix = R.split_pixels(self.c, splits, mps, R_rows).cuda()
            self._split[key] = torch.stack([self._ref(pix[s]) for s in range(splits)], 1)  # [G, splits, Co, taps, Cs]
        return self._split[key]

    def args(self, slab, splits, mps):
        c = self.c
        Pi = c.B * c.H * c.W
        src = {"p0": P(self.buf0, c.off0), "ld0": c.ld0, "C0": c.C0, "C1": c.C1, "gs0": Pi * c.ld0 + c.gap}
        if c.C1:
            src.update(p1=P(self.buf1, c.off1), ld1=c.ld1, gs1=Pi * c.ld1 + c.gap)
        d = {"src": src, "dy": P(self.dybuf, c.doff), "dgs": c.M * c.ldd + c.gap, "ldd": c.ldd, "slab": P(slab),
             "splits": splits, "m_per_split": mps, "B": c.B, "Hi": c.H, "Wi": c.W, "Ho": c.Ho, "Wo": c.Wo, "Co": c.Co,
             "Npad": c.Npad, "Cs": c.Cs, "KH": c.KH, "KW": c.KW, "sh": c.sh, "sw": c.sw, "ph": c.ph, "pw": c.pw,
             "Kpad": c.Kpad}
        if c.nol is not None:
            d["nol"] = {"consts": P(self.consts), "kind": c.nol}
        return d

    def slab(self, splits):
        c = self.c
        return self.bufs.fill((c.G, splits, c.Npad, c.Kpad), torch.float32, R.SENT, "slab")

    def check(self, chk, what, slab, splits, mps, R_rows):
        """The slab [G, splits, Npad, Kpad] against the references: per split (integer cases) and summed."""
        c = self.c
        got = slab[:, :, :c.Co, :c.taps * c.Cs].reshape(c.G, splits, c.Co, c.taps, c.Cs)
        if c.real:
            chk.wgrad_real(what, got.double().sum(1), self.ref, self.T, c.M)
            return
        chk.exact(what + " per split", got, self.split_ref(splits, mps, R_rows))
        chk.exact(what + " summed", got.sum(1), self.ref)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = WProblem(c)
        return cache[c.name]
    return get


def _valid(fn, cfg, c):
    if cfg in fn.WGRAD_PATCH:
        return fn.patch_valid(cfg, c.Cs, c.KH, c.KW, (c.sh, c.sw), (c.ph, c.pw), c.H, c.W, c.Ho, c.Wo, c.C0, c.C1)
    return fn.wgrad_ktiles(cfg, c.Kpad) > 0


def _engine_plan(core, cfg, c):
    """ConvLayer.wgrad_plan on this case's geometry."""
    L = core.ConvLayer
    ns = types.SimpleNamespace(B=c.B, Ho=c.Ho, Npad=c.Npad, Cs=c.Cs, G=c.G, Kpad_w=c.Kpad, M_out=c.M,
                               MIN_SPLIT_PX=L.MIN_SPLIT_PX, MIN_SPLIT_PX_BIG=L.MIN_SPLIT_PX_BIG,
                               LEAN_MIN_CHUNKS=L.LEAN_MIN_CHUNKS, LEAN_BLOCKS=L.LEAN_BLOCKS,
                               LEAN_MAX_SPLITS=L.LEAN_MAX_SPLITS)
    return L.wgrad_plan(ns, cfg)


def _plans(fn, core, cfg, c):
    """[(name, splits, m_per_split)] and the strip rows of a patch config (0: pixel units)."""
    if cfg in fn.WGRAD_PATCH:
        R_rows = fn.WGRAD_PATCH[cfg][3]
        U = c.B * math.ceil(c.Ho / R_rows)
        forced = [("short last", 2, U - 1), ("one split", 1, U)]
    else:
        R_rows = 0
        (s1, m1), (s2, m2) = R.forced_plans(c.M, fn.WGRAD_TILES[cfg][2])
        forced = [("short last", s1, m1), ("one split", s2, m2)]
    return [("engine",) + tuple(_engine_plan(core, cfg, c))] + forced, R_rows


@pytest.mark.parametrize("family", list(FAMILIES))
def test_wgrad_forms(fn, core, problems, family):
    chk, ran, which = R.Checker(), 0, {}
    for c in R.WCASES:
        pr = problems(c)
        for cfg in FAMILIES[family]:
            if not _valid(fn, cfg, c):
                continue
            plans, R_rows = _plans(fn, core, cfg, c)
            for name, splits, mps in plans:
                slab = pr.slab(splits)
                _lib().wgrad(cfg, c.G, _stream(), pr.args(slab, splits, mps))
                pr.check(chk, f"{c.name} cfg {cfg} {name} ({splits} x {mps})", slab, splits, mps, R_rows)
            ran += 1
            which.setdefault(c.name, []).append(cfg)
        pr.bufs.check(chk)
        pr.drop_slabs()
    print("configs per case", which)
    assert ran >= MIN_RAN[family], (ran, which)
    chk.done()


def _batch_plan(fn, core, cfg, c):
    """The short-last-split plan where the map has more than one chunk (more blocks than the caps), else the
    engine's."""
    if cfg in fn.WGRAD_PATCH:
        return 2, c.B * math.ceil(c.Ho / fn.WGRAD_PATCH[cfg][3]) - 1
    MCH = fn.WGRAD_TILES[cfg][2]
    return R.forced_plans(c.M, MCH)[0] if c.M > MCH and c.M % MCH else _engine_plan(core, cfg, c)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_wgrad_batched(fn, core, problems, family):
    """One table of heterogeneous jobs per config, uncapped and on a capped persistent grid: every job's slab is
    bit-identical to its own per-conv launch and equals the reference."""
    chk, nbatch = R.Checker(), 0
    pool = R.WBATCH_PATCH if family == "patch" else R.WBATCH_IM2COL
    for cfg in FAMILIES[family]:
        jobs = [problems(c) for c in pool if _valid(fn, cfg, c)]
        if len(jobs) < 2:
            continue
        R_rows = fn.WGRAD_PATCH[cfg][3] if cfg in fn.WGRAD_PATCH else 0
        plans = [_batch_plan(fn, core, cfg, pr.c) for pr in jobs]
        own = []
        for pr, (splits, mps) in zip(jobs, plans):
            slab = pr.slab(splits)
            _lib().wgrad(cfg, pr.c.G, _stream(), pr.args(slab, splits, mps))
            pr.check(chk, f"{pr.c.name} cfg {cfg} per-conv", slab, splits, mps, R_rows)
            own.append(slab)
        for cap in (0, 3, 7):
            slabs = [pr.slab(s) for pr, (s, _) in zip(jobs, plans)]
            raw, nblocks = _lib().wgrad_table(cfg, [pr.args(sl, s, m) for pr, sl, (s, m) in zip(jobs, slabs, plans)],
                                              [pr.c.G for pr in jobs])
            t = table(raw)
            chk.true(f"cfg {cfg}: the table holds more blocks than either cap", nblocks > 7 or len(jobs) < 4)
            _lib().wgrad_batched(cfg, P(t), len(jobs), nblocks, _stream(), cap)
            for pr, a, b in zip(jobs, own, slabs):
                chk.exact(f"{pr.c.name} cfg {cfg} cap {cap} batched == per-conv", b.view(torch.int32), a.view(torch.int32))
        nbatch += len(jobs) >= 4
        for pr in jobs:
            pr.bufs.check(chk)
            pr.drop_slabs()
    assert nbatch >= MIN_BATCH[family], nbatch
    chk.done()


# ---------------------------------------------------------------------------------------------------
# B. wgrad_finalize
class FinProblem:
    """The slabs of R.fin_descs(rot) on the device, the gradient buffer's layout and the fp64 expectation."""

    def __init__(self, rot):
        self.descs = R.fin_descs(rot)
        self.bufs = Bufs()
        self.slabs_cpu = [R.fin_slab(d, 100 * rot + i) for i, d in enumerate(self.descs)]
        self.slabs = [self.bufs.put(s, "slab " + d["name"]) for s, d in zip(self.slabs_cpu, self.descs)]
        pos, self.where = 24, []
        for d in self.descs:
            for mem in d["members"]:
                n = mem[0] * d["Ci"] * mem[1] * mem[2]
                ggs = n + R.FIN_GGS_EXTRA if d["G"] > 1 else 0
                self.where.append((pos, ggs))
                pos += (d["G"] - 1) * ggs + n + 24
        self.numel = pos

    def expected(self, scale):
        out = torch.full((self.numel,), R.SENT, dtype=torch.float64)
        it = iter(self.where)
        for d, slab in zip(self.descs, self.slabs_cpu):
            for mem in d["members"]:
                off, ggs = next(it)
                ref = R.fin_ref(slab, d, mem, scale)
                for g in range(d["G"]):
                    out[off + g * ggs:off + g * ggs + ref[g].numel()] = ref[g].reshape(-1)
        return out

    def table_descs(self, grad):
        out, it = [], iter(self.where)
        for d, slab in zip(self.descs, self.slabs):
            for Co, kh, kw, n0, t0 in d["members"]:
                off, ggs = next(it)
                out.append({"slab": P(slab, n0 * d["Kpad"] + t0 * d["Cs"]), "grad": P(grad, off), "ggs": ggs, "G": d["G"],
                            "splits": d["splits"], "Npad": d["Npad"], "Kpad": d["Kpad"], "Co": Co, "Ci": d["Ci"],
                            "Cs": d["Cs"], "KH": kh, "KW": kw, "elems": d["G"] * Co * d["Ci"] * kh * kw})
        return out


@pytest.fixture(scope="module")
def fin_problems():
    cache = {}

    def get(rot):
        if rot not in cache:
            cache[rot] = FinProblem(rot)
        return cache[rot]
    return get


# rotations of the split counts over the shapes under which every shape is finalized in output order (<= 8 splits)
# at least once and with many splits at least once
FIN_ROTS = [0, 1, 2, 5, 9]


@pytest.mark.parametrize("rot", FIN_ROTS)
@pytest.mark.parametrize("max_out", [0, 2, 8])
def test_wgrad_finalize(core, fin_problems, monkeypatch, max_out, rot):
    monkeypatch.setattr(core, "FIN_OUT_MAX_SPLITS", max_out)
    chk, pr = R.Checker(), fin_problems(rot)
    for scale in (1.0, 0.125):
        grad = pr.bufs.fill((pr.numel,), torch.float32, R.SENT, "grad")
        descs = pr.table_descs(grad)
        t, nd, nblocks = core.build_wgfin_table(descs, "cuda")
        _lib().wgrad_finalize(P(t), nd, nblocks, scale, _stream())
        exp = pr.expected(scale).cuda()
        if not chk.exact(f"finalize scale {scale}", grad, exp):
            it = iter(pr.where)  # name the descriptor
            for d in pr.descs:
                for mem in d["members"]:
                    off, ggs = next(it)
                    n = (d["G"] - 1) * ggs + mem[0] * d["Ci"] * mem[1] * mem[2]
                    if not torch.equal(grad[off:off + n].double(), exp[off:off + n]):
                        chk.bad.append((d["name"], mem, "splits", d["splits"], "lanes", core.finalize_lanes(d["splits"]),
                                        "order", int(d["splits"] <= max_out)))
    pr.bufs.check(chk)
    pr.bufs.all = pr.bufs.all[:len(pr.slabs)]
    chk.done()


# ---------------------------------------------------------------------------------------------------
# C. adam_pack
class OptProblem:
    def __init__(self, core, seed):
        self.numel, self.images = R.opt_layout()
        self.bufs = Bufs()
        self.cpu = dict(zip("pgmv", R.adam_state(self.numel, seed)))
        self.dev = {k: self.bufs.put(v, k) for k, v in self.cpu.items()}
        self.lr = self.bufs.put(torch.tensor([1e-3]), "lr")
        self.step = self.bufs.put(torch.tensor([0.0]), "step")
        self.cursor = self.bufs.put(torch.tensor([5], dtype=torch.int64), "cursor")
        # images: zero where a member writes or must keep zeros, the sentinel in the padding nobody writes
        self.fill_f, self.fill_d, self.wf, self.wd, conv_segs = [], [], [], [], []
        for im in self.images:
            taps = im["KH"] * im["KW"]
            ff = torch.full((im["Npad"], im["Kpad"]), R.SENT).bfloat16()
            ff[:im["Co"], :taps * im["Cs"]] = 0
            fd = torch.full((im["Npad_d"], im["Kpad_d"]), R.SENT).bfloat16()
            fd[:im["Ci"], :taps * im["Co"]] = 0
            self.fill_f.append(ff)
            self.fill_d.append(fd)
            self.wf.append(self.bufs.put(ff, "wf " + im["name"]))
            self.wd.append(self.bufs.put(fd, "wd " + im["name"]))
            fused = len(im["members"]) > 1
            for Co, kh, kw, n0, t0, off in im["members"]:  # the dict shapes of ConvLayer.opt_segments
                s = {"kind": 3, "off": off, "n": Co * im["Ci"] * kh * kw, "Co": Co, "Ci": im["Ci"], "KH": kh, "KW": kw,
                     "Cs": im["Cs"], "Kpad_f": im["Kpad"], "Kpad_d": im["Kpad_d"],
                     "wf": P(self.wf[-1], n0 * im["Kpad"] + t0 * im["Cs"]), "wd": P(self.wd[-1], t0 * im["Co"] + n0)}
                if fused:
                    s.update(tap_ld=im["Co"], kext_f=kh * kw * im["Cs"] if t0 else 0)
                conv_segs.append(s)
        self.conv_segs = conv_segs
        self.segs = core.optimizer_segments(conv_segs, self.numel)
        self.table = core.build_optseg_table(self.segs, "cuda")

    def reset(self, step, cursor=5):
        for k, v in self.cpu.items():
            self.dev[k].copy_(v)
        for i in range(len(self.images)):
            self.wf[i].copy_(self.fill_f[i])
            self.wd[i].copy_(self.fill_d[i])
        self.step.fill_(float(step))
        self.cursor.fill_(cursor)

    def launch(self, tab=None, **kw):
        t, ns, nblocks = tab or self.table
        d = {"p": P(self.dev["p"]), "g": P(self.dev["g"]), "m": P(self.dev["m"]), "v": P(self.dev["v"]), "n": self.numel,
             "lr": P(self.lr), "step": P(self.step), "segs": P(t), "nsegs": ns, "nblocks": nblocks}
        d.update(kw)
        _lib().adam_pack(_stream(), d)

    def state(self):
        return {k: v.cpu().clone() for k, v in self.dev.items()}

    def check_images(self, chk, what):
        p = self.dev["p"].cpu()
        for i, im in enumerate(self.images):
            wf, wd = R.image_refs(im, p, self.fill_f[i], self.fill_d[i])
            chk.bits(f"{what}: forward image {im['name']}", self.wf[i], wf)
            chk.bits(f"{what}: data-gradient image {im['name']}", self.wd[i], wd)


@pytest.fixture(scope="module")
def opt(core):
    return OptProblem(core, 1)


def _bits_same(chk, what, a, b):
    for k in "pmv":
        chk.exact(f"{what}: {k} bit-unchanged", a[k].view(torch.int32), b[k].view(torch.int32))


def test_adam_pack_only(opt):
    """update = 0: p, m, v, step and cursor bit-unchanged, the images rebuilt from p."""
    chk = R.Checker()
    opt.reset(9)
    opt.launch(update=0, cursor=P(opt.cursor))
    _bits_same(chk, "pack only", opt.state(), opt.cpu)
    chk.true("step unchanged", float(opt.step) == 9.0 and int(opt.cursor) == 5)
    opt.check_images(chk, "pack only")
    opt.bufs.check(chk)
    chk.done()


@pytest.mark.parametrize("step0,wd,gs", [(0, 0.0, 1.0), (0, 1e-5, 0.125), (1, 1e-5, 1.0), (9, 0.0, 0.125),
                                         (9, 1e-5, 0.125), (9999, 1e-5, 1.0), (9999, 0.0, 0.125)])
@pytest.mark.parametrize("mode", ["inc", "noinc", "t_pre"])
def test_adam_pack_update(opt, mode, step0, wd, gs):
    if mode == "t_pre" and step0 == 0:
        step0 = 1  # the early increment has already run: the counter is at least 1
    chk = R.Checker()
    opt.reset(step0)
    kw = {"inc": dict(inc_step=1), "noinc": dict(inc_step=0), "t_pre": dict(inc_step=0, t_pre=1)}[mode]
    opt.launch(update=1, wd=wd, grad_scale=gs, cursor=P(opt.cursor), **kw)
    t = step0 if mode == "t_pre" else step0 + 1
    got = opt.state()
    chk.adam(f"{mode} t {t} wd {wd} grad_scale {gs}", got, opt.cpu, t, float(opt.lr), wd=wd, grad_scale=gs)
    chk.exact("gradient untouched", got["g"].view(torch.int32), opt.cpu["g"].view(torch.int32))
    inc = 1 if mode == "inc" else 0
    chk.true("step counter and cursor", float(opt.step) == step0 + inc and int(opt.cursor) == 5 + inc)
    opt.check_images(chk, mode)
    opt.bufs.check(chk)
    chk.done()


def test_adam_pack_partial_updates(core, opt):
    """The conv segments of some weights in an early launch (inc_step = 0), the rest in a second one: bit-identical
    state, images and counters to one launch."""
    chk = R.Checker()
    hp = dict(update=1, wd=1e-5, grad_scale=0.125)
    opt.reset(9)
    opt.launch(inc_step=1, cursor=P(opt.cursor), **hp)
    one = opt.state()
    imgs = [(a.clone(), b.clone()) for a, b in zip(opt.wf, opt.wd)]
    early = {s["off"] for s in opt.conv_segs[::2]}
    t1 = core.build_optseg_table([s for s in opt.segs if s["kind"] == 3 and s["off"] in early], "cuda")
    t2 = core.build_optseg_table([s for s in opt.segs if not (s["kind"] == 3 and s["off"] in early)], "cuda")
    opt.reset(9)
    opt.launch(t1, inc_step=0, **hp)
    chk.true("the early launch leaves the counters", float(opt.step) == 9.0 and int(opt.cursor) == 5)
    opt.launch(t2, inc_step=1, cursor=P(opt.cursor), **hp)
    _bits_same(chk, "two launches", opt.state(), one)
    for i, (a, b) in enumerate(imgs):
        chk.bits(f"forward image {i}", opt.wf[i], a)
        chk.bits(f"data-gradient image {i}", opt.wd[i], b)
    chk.true("counters", float(opt.step) == 10.0 and int(opt.cursor) == 6)
    opt.bufs.check(chk)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# D. the packed-tap stem
B_STEM, N_STEM, NROWS, CO_STEM = 3, 7, 4, 16


class Stem:
    def __init__(self, core, spec, integer):
        KH, KW, s, p, H, W = spec
        self.spec, self.bufs = spec, Bufs()
        self.conv = torch.nn.Conv2d(1, CO_STEM, (KH, KW), stride=s, padding=p, bias=False)
        self.geom = core.stem_pack_geom(self.conv, H, W)
        assert self.geom is not None
        g = R.gen(4000 + KH)
        if integer:
            self.X = R.ints(g, (N_STEM, 1, H, W), 1, 0.3)
            self.w = R.ints(g, (CO_STEM, 1, KH, KW), 2, 0.1)
        else:
            self.X = torch.randn(N_STEM, 1, H, W, generator=g)
            self.w = torch.randn(CO_STEM, 1, KH, KW, generator=g) / math.sqrt(KH * KW)
        self.lab = torch.randint(0, 9, (N_STEM, 2), generator=g)
        self.idx = torch.stack([torch.randperm(N_STEM, generator=g)[:B_STEM] for _ in range(NROWS)])  # [nrows][B]
        self.dX, self.dlab, self.didx = self.bufs.put(self.X, "X"), self.bufs.put(self.lab, "labels"), self.bufs.put(self.idx, "idx")

    def gather(self, cursor_value, zero=()):
        KH, KW, s, p, H, W = self.spec
        out = self.bufs.fill((B_STEM, H, W, 8), torch.bfloat16, R.SENT, "packed batch")
        lab = self.bufs.fill((B_STEM, 2), torch.int64, -7, "gathered labels")
        cur = self.bufs.put(torch.tensor([cursor_value], dtype=torch.int64), "cursor")
        from mtl_das_pytorch_amd.ops.functional import gather_args
        # (the launch dict on this case's guarded buffers: functional.gather_batch allocates its own labels)
        d = gather_args(X=self.dX, labels=self.dlab, lab_w=2, idx=self.didx, out=out, lab_out=lab, B=B_STEM, H=H, W=W,
                        taps=self.geom["taps"], off=self.geom["off"], zero=list(zero), cursor=cur)
        assert d["nrows"] == NROWS and d["Cin"] == 1
        _lib().gather_batch(_stream(), d)
        return out, lab, self.idx[cursor_value % NROWS]


@pytest.mark.parametrize("spec", R.STEMS)
def test_stem_gather(core, spec):
    chk, st = R.Checker(), Stem(core, spec, integer=False)
    z1 = st.bufs.fill((48,), torch.float32, R.SENT, "zero range 1")
    z2 = st.bufs.fill((20,), torch.float64, R.SENT, "zero range 2")
    for cv in (0, 1, NROWS + 1):
        z1.fill_(3.0)
        z2.fill_(3.0)
        out, lab, idx = st.gather(cv, [(P(z1, 4), 32 * 4), (P(z2, 2), 16 * 8)])
        chk.bits(f"cursor {cv}: packed batch", out, R.pack_taps_ref(st.X, idx, st.geom["taps"], st.geom["off"]))
        chk.exact(f"cursor {cv}: labels", lab, st.lab[idx])
        chk.true("zero ranges zeroed inside, untouched outside",
                 bool((z1[4:36] == 0).all() and (z1[:4] == 3).all() and (z1[36:] == 3).all()
                      and (z2[2:18] == 0).all() and (z2[:2] == 3).all() and (z2[18:] == 3).all()))
    st.bufs.check(chk)
    chk.done()


def _stem_case(st, real=False):
    """The virtual 1 x KW convolution over the packed input as a WCase (Ho, Wo: the real convolution's)."""
    KH, KW, s, p, H, W = st.spec
    g = st.geom
    c = R.WCase("stem", B_STEM, H, W, 8, CO_STEM, KH=g["KH"], KW=g["KW"], sh=g["sh"], sw=g["sw"], ph=g["ph"], pw=g["pw"])
    c.Ho, c.Wo = g["Ho"], g["Wo"]
    return c


@pytest.mark.parametrize("spec", R.STEMS)
def test_stem_wgrad_chain(fn, core, spec):
    """gather (packed taps) -> wgrad with the virtual geometry -> finalize == the fp64 weight gradient of the REAL
    KH x KW convolution on the unpacked input, exactly (integer data)."""
    chk, st = R.Checker(), Stem(core, spec, integer=True)
    KH, KW, s, p, H, W = spec
    x, _, idx = st.gather(1)
    c = _stem_case(st)
    dy = R.ints(R.gen(5), (B_STEM, c.Ho, c.Wo, CO_STEM))
    ddy = st.bufs.put(dy.bfloat16(), "dy")
    real = R.WCase("real", B_STEM, H, W, 1, CO_STEM, KH=KH, KW=KW, sh=s, sw=s, ph=p, pw=p)
    assert (real.Ho, real.Wo) == (c.Ho, c.Wo)
    ref = R.to_nchw(R.wgrad_ref(st.X[idx].permute(0, 2, 3, 1).double(), dy.double(), real), real)   # [Co, 1, KH, KW]
    ran = 0
    for cfg in list(fn.WGRAD_TILES):
        if not fn.wgrad_ktiles(cfg, c.Kpad):
            continue
        splits, mps = _engine_plan(core, cfg, c)
        if splits == 1 and c.M > fn.WGRAD_TILES[cfg][2]:
            splits, mps = R.forced_plans(c.M, fn.WGRAD_TILES[cfg][2])[0]
        slab = st.bufs.fill((1, splits, c.Npad, c.Kpad), torch.float32, R.SENT, "slab")
        d = {"src": {"p0": P(x), "ld0": 8, "C0": 8, "C1": 0}, "dy": P(ddy), "ldd": CO_STEM, "slab": P(slab),
             "splits": splits, "m_per_split": mps, "B": B_STEM, "Hi": H, "Wi": W, "Ho": c.Ho, "Wo": c.Wo, "Co": CO_STEM,
             "Npad": c.Npad, "Cs": 8, "KH": 1, "KW": KW, "sh": c.sh, "sw": c.sw, "ph": 0, "pw": c.pw, "Kpad": c.Kpad}
        _lib().wgrad(cfg, 1, _stream(), d)
        grad = st.bufs.fill((24 + ref.numel() + 24,), torch.float32, R.SENT, "grad")
        desc = {"slab": P(slab), "grad": P(grad, 24), "ggs": 0, "G": 1, "splits": splits, "Npad": c.Npad, "Kpad": c.Kpad,
                "Co": CO_STEM, "Ci": KH, "Cs": 8, "KH": 1, "KW": KW, "elems": ref.numel()}
        t, nd, nblocks = core.build_wgfin_table([desc], "cuda")
        _lib().wgrad_finalize(P(t), nd, nblocks, 1.0, _stream())
        exp = torch.full((grad.numel(),), R.SENT, dtype=torch.float64)
        exp[24:24 + ref.numel()] = ref.reshape(-1)
        chk.exact(f"stem {spec} cfg {cfg} ({splits} splits)", grad, exp)
        ran += 1
    assert ran >= 24, ran  # configs 0-7 (TK 32 / 64 divide Kpad = 64) and the 16 big / lean ones (partial K tile)
    st.bufs.check(chk)
    chk.done()


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("spec", R.STEMS)
def test_stem_forward_chain(fn, core, spec, integer):
    """adam_pack (update = 0) on the real weight builds the virtual image; the forward conv on the packed input is
    the real convolution."""
    chk, st = R.Checker(), Stem(core, spec, integer)
    KH, KW, s, p, H, W = spec
    x, _, idx = st.gather(2)
    c = _stem_case(st)
    n = st.w.numel()
    flat = st.bufs.put(torch.cat([torch.full((8,), 0.5), st.w.reshape(-1), torch.full((4,), 0.5)]), "flat")
    Kpad, Kpad_d = R.pad_to(KW * 8, 32), R.pad_to(KW * CO_STEM, 32)
    wf = st.bufs.fill((c.Npad, Kpad), torch.bfloat16, 0, "wf")
    wd = st.bufs.fill((16, Kpad_d), torch.bfloat16, 0, "wd")
    seg = {"kind": 3, "off": 8, "n": n, "Co": CO_STEM, "Ci": KH, "KH": 1, "KW": KW, "Cs": 8, "Kpad_f": Kpad,
           "Kpad_d": Kpad_d, "wf": P(wf), "wd": P(wd)}
    t, ns, nblocks = core.build_optseg_table(core.optimizer_segments([seg], flat.numel()), "cuda")
    _lib().adam_pack(_stream(), {"p": P(flat), "g": 0, "m": 0, "v": 0, "n": flat.numel(), "lr": 0, "step": 0, "update": 0,
                                 "segs": P(t), "nsegs": ns, "nblocks": nblocks})
    chk.bits("virtual forward image", wf, fn.pack_weight_fwd(st.w.view(CO_STEM, KH, 1, KW), 8))
    y = st.bufs.fill((B_STEM, c.Ho, c.Wo, CO_STEM), torch.bfloat16, R.SENT, "y")
    d = {"src": {"p0": P(x), "ld0": 8, "C0": 8, "C1": 0}, "w": P(wf), "out": P(y), "ldo": CO_STEM, "B": B_STEM, "Hs": H,
         "Ws": W, "Ho": c.Ho, "Wo": c.Wo, "N": CO_STEM, "Npad": c.Npad, "Cs": 8, "KH": 1, "KW": KW, "sh": c.sh,
         "sw": c.sw, "ph": 0, "pw": c.pw, "Kpad": Kpad}
    _lib().conv(0, 0, 1, _stream(), d)
    xb, wb = st.X[idx].bfloat16().double(), st.w.bfloat16().double()
    ref = torch.nn.functional.conv2d(xb, wb, stride=s, padding=p).permute(0, 2, 3, 1)
    if integer:
        assert float(ref.abs().max()) <= 98
        chk.exact(f"stem {spec} forward", y, ref)
    else:
        chk.bounded("stem forward", f"stem {spec}", y, ref, ref.abs() * 2.0 ** -8 + 1e-5 * ref.abs().max())
    st.bufs.check(chk)
    chk.done()
