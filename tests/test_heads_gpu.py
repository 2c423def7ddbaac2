"""Task heads and on-device metrics (csrc/head.hip) against fp64 references (MI355X only).

``mtl_head`` (Models A/B) and ``cls_head`` + ``cls_wgrad`` (Model C) produce every reported number -- loss,
accuracy, distance MAE, the confusion matrices -- and the first gradient of every backward pass.  Inputs are
rounded to bf16 first and the references are computed in fp64 from the rounded values: the GAP and the group
means are cancelling sums, so the tolerances below absorb only the kernels' fp32 accumulation, their fast
exp / log, and the single bf16 rounding of the stored gradients.  Integer quantities (counts, |pred - label|,
confusion matrices) are compared exactly; the generators keep every prediction away from a tie so that
"exactly" is well defined.  The last section drives the evaluation phase of each lowered program the way
EngineBackend.eval_batch does and recomputes the device metrics from the program's own log-probabilities.

No test passes an out-of-range label, and every argument set that is expected to be refused is refused on the
host before a kernel is launched."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
CANARY = 7.0        # exact in bf16 and fp32
ICANARY = -123      # confusion-matrix canary


def _lib():
    from mtl_das_pytorch_amd.ops.hip import lib
    return lib()


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def rel64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """bf16 tensor -> int16 bit patterns (numpy)."""
    return _np(t.view(torch.int16))


def _log_softmax64(z):
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def _top2_margin(z):
    s = np.sort(z, -1)
    return s[..., -1] - s[..., -2]


def _confusion(lab, pred):
    cm = np.zeros((16, 16), np.int64)
    np.add.at(cm, (lab, pred), 1)
    return cm


# =====================================================================================================
# A. mtl_head (Models A/B)
# =====================================================================================================
MTL_SHAPES = [
    # T, B, HW, C, ncls                  GAP loop: lanes = 256 / (C/8), unrolled while p + 3*lanes < HW
    (1, 3, 1, 8, [2]),                 # one 8-channel group, 256 lanes, one pixel, group size 4 (the minimum)
    (4, 5, 7, 64, [16, 8, 4, 2]),      # T at its limit, HW < lanes (tail loop only), four group sizes
    (2, 4, 35, 256, [16, 2]),          # C at its maximum, lanes = 8, HW = 4*lanes + 3
    (2, 2, 149, 128, [16, 2]),         # two unrolled rounds plus a partial tail
    (2, 6, 55, 128, [16, 2]),          # the shape of test_kernels_gpu.py::test_mtl_head
]
MTL_W = [1.0, 0.5, 2.0, 0.25]
_ORDER = {True: [1, 2, 0], False: [0, 1, 2]}  # 0: right, 1: label < pred, 2: label > pred


class MtlCase:
    """Inputs of one mtl_head launch (built on the host), their fp64 reference, and the device buffers."""

    def __init__(self, T, B, HW, C, ncls, seed=0, padded=False, lab_stride=None, lab_off=0, const=False):
        self.T, self.B, self.HW, self.C, self.ncls = T, B, HW, C, list(ncls)
        self.w = MTL_W[:T]
        rng = np.random.default_rng(seed)
        g = torch.Generator().manual_seed(seed)
        # classes: per (b, t) one of right / label < pred / label > pred (two classes: right / wrong either way)
        order = _ORDER[B < 3]
        self.boost = np.zeros((B, T), np.int64)
        self.lab = np.zeros((B, T), np.int64)
        for b in range(B):
            for t in range(T):
                K = ncls[t]
                kind = order[(b + t) % 3]
                if kind == 0:
                    p = int(rng.integers(0, K)); l = p
                elif kind == 1:
                    p = int(rng.integers(1, K)); l = int(rng.integers(0, p))
                else:
                    p = int(rng.integers(0, K - 1)); l = int(rng.integers(p + 1, K))
                self.boost[b, t], self.lab[b, t] = p, l
        if const:  # every logit bit-equal: the prediction is the first maximum
            feat = torch.full((T, B, HW, C), 0.25)
        else:
            feat = 0.5 * torch.randn(T, B, HW, C, generator=g)
            for b in range(B):
                for t in range(T):
                    gsz = C // ncls[t]
                    feat[t, b, :, self.boost[b, t] * gsz:(self.boost[b, t] + 1) * gsz] += 2.0
        feat = feat.bfloat16()
        self.feat64 = feat.double().numpy()
        # device layout
        self.ldf = C + 8 if padded else C
        self.fgs = B * HW * self.ldf + (16 if padded else 0)
        fb = torch.full((T, self.fgs), NAN if padded else 0.0, dtype=torch.bfloat16)
        fb[:, :B * HW * self.ldf].view(T, B * HW, self.ldf)[:, :, :C] = feat.view(T, B * HW, C)
        self.fb = fb.to(DEV)
        # padded: a label pitch of 3 (of T + 1 at T = 4: a pitch below T would alias the next row's labels)
        self.lab_stride = lab_stride if lab_stride is not None else (max(3, T + 1) if padded else T)
        self.lab_off = lab_off
        assert self.lab_off + T <= self.lab_stride
        # columns the kernel must not read hold a valid class that differs from every label of the row
        lb = np.repeat(1 - (self.lab[:, :1] % 2), self.lab_stride, axis=1)
        lb[:, lab_off:lab_off + T] = self.lab
        self.labels = torch.from_numpy(lb).to(DEV)
        self.dgs = B * HW * C + (8 if padded else 0)
        self._reference()
        self.reset()

    def _reference(self):
        T, B, HW, C = self.T, self.B, self.HW, self.C
        gap = self.feat64.mean(2)  # [T, B, C]
        self.logits, self.logp_ref, self.pred, self.nll = [], [], [], []
        self.dfeat_ref = np.zeros((T, B, HW, C))
        for t, K in enumerate(self.ncls):
            gsz = C // K
            z = gap[t].reshape(B, K, gsz).mean(-1)
            lp = _log_softmax64(z)
            self.logits.append(z)
            self.logp_ref.append(lp)
            self.pred.append(z.argmax(-1))  # first maximum, as torch.argmax documents
            self.nll.append(-lp[np.arange(B), self.lab[:, t]])
            d = np.exp(lp)
            d[np.arange(B), self.lab[:, t]] -= 1.0
            d *= self.w[t] / (B * gsz * HW)
            self.dfeat_ref[t] = np.repeat(d, gsz, axis=1)[:, None, :]

    def min_margin(self):
        return min(float(_top2_margin(z).min()) for z in self.logits)

    def reset(self):
        T, B = self.T, self.B
        self.logp = torch.full((T, B, 16), CANARY, device=DEV)
        self.dfeat = torch.full((T, self.dgs), CANARY, device=DEV, dtype=torch.bfloat16)
        self.metrics = torch.zeros(T, 4, device=DEV)
        self.conf = torch.zeros(T, 16, 16, device=DEV, dtype=torch.int32)

    def args(self, train=True, nvalid=None, **over):
        d = {"feat": _ptr(self.fb), "fgs": self.fgs, "ldf": self.ldf, "labels": _ptr(self.labels),
             "lab_stride": self.lab_stride, "lab_off": self.lab_off, "T": self.T, "B": self.B, "HW": self.HW,
             "C": self.C, "ncls": list(self.ncls), "w": list(self.w), "logp": _ptr(self.logp),
             "dfeat": _ptr(self.dfeat) if train else 0, "dgs": self.dgs, "metrics": _ptr(self.metrics),
             "confusion": _ptr(self.conf)}
        if nvalid is not None:
            d["nvalid"] = _ptr(nvalid)
        d.update(over)
        return d

    def launch(self, **kw):
        _lib().mtl_head(_stream(), self.args(**kw))
        _sync()

    # ---- checks -------------------------------------------------------------------------------------
    def expected_metrics(self, nv=None, times=1):
        nv = self.B if nv is None else nv
        met = np.zeros((self.T, 4))
        cm = np.zeros((self.T, 16, 16), np.int64)
        for t in range(self.T):
            l, p = self.lab[:nv, t], self.pred[t][:nv]
            met[t] = [self.nll[t][:nv].sum(), (l == p).sum(), nv, np.abs(p - l).sum()]
            cm[t] = _confusion(l, p)
        return met * times, cm * times

    def check_logp(self):
        lp = _np(self.logp).astype(np.float64)
        err = 0.0
        for t, K in enumerate(self.ncls):
            err = max(err, float(np.abs(lp[t, :, :K] - self.logp_ref[t]).max()))
        print(f"mtl_head logp max abs err {err:.3e}")
        assert np.isfinite(lp).all()
        assert err < 1e-4, err

    def check_metrics(self, nv=None, times=1):
        met, cm = self.expected_metrics(nv, times)
        got = _np(self.metrics).astype(np.float64)
        for t in range(self.T):
            e = abs(got[t, 0] - met[t, 0]) / max(abs(met[t, 0]), 1e-300) if met[t, 0] else abs(got[t, 0])
            print(f"mtl_head task {t} loss sum rel err {e:.3e}")
            assert e < 1e-4, (t, got[t, 0], met[t, 0])
        assert np.array_equal(got[:, 1:], met[:, 1:]), (got, met)
        assert np.array_equal(_np(self.conf).astype(np.int64), cm)  # rows = label, columns = prediction

    def check_dfeat(self):
        T, B, HW, C = self.T, self.B, self.HW, self.C
        body = self.dfeat[:, :B * HW * C]
        d = _np(body.float()).astype(np.float64).reshape(T, B, HW, C)
        e = rel64(d, self.dfeat_ref)
        print(f"mtl_head dfeat rel L2 err {e:.3e}")
        assert e < 4e-3, e  # one bf16 rounding
        assert (_np(self.dfeat[:, B * HW * C:].float()) == CANARY).all()  # the gap between the task groups
        bits = _bits(body.contiguous()).reshape(T, B, HW, C)
        assert (bits == bits[:, :, :1]).all(), "dfeat differs between the pixels of one sample"
        for t, K in enumerate(self.ncls):
            gsz = C // K
            bg = bits[t].reshape(B, HW, K, gsz)
            assert (bg == bg[..., :1]).all(), "dfeat differs inside one class group"
            neg = d[t].reshape(B, HW, K, gsz) < 0
            want = (np.arange(K)[None, :] == self.lab[:, t][:, None])[:, None, :, None]
            assert np.array_equal(neg, np.broadcast_to(want, neg.shape)), "dfeat sign: negative exactly on the label"


def _mtl_layouts():
    out = []
    for i, s in enumerate(MTL_SHAPES):
        for padded in (False, True):
            out.append(pytest.param(s, padded, 100 + i, id=f"{'x'.join(map(str, s[:4]))}-{'padded' if padded else 'dense'}"))
    return out


@pytest.mark.parametrize("shape,padded,seed", _mtl_layouts())
def test_mtl_head_reference(shape, padded, seed):
    """logp, metrics, confusion and dfeat at every path of the GAP loop; ``padded``: ldf = C + 8, a gap after
    each task's features and gradients (NaN / canary), and a label pitch wider than the task count."""
    c = MtlCase(*shape, seed=seed, padded=padded)
    assert c.min_margin() > 0.5, f"generator seed {seed}: top-two logit margin {c.min_margin()}"
    for t, K in enumerate(c.ncls):  # the generator covers right / wrong in both directions
        l, p = c.lab[:, t], c.pred[t]
        assert np.array_equal(p, c.boost[:, t])
        if K > 2 and c.B >= 2:
            assert (l < p).any() and (l > p).any()
    assert any((c.lab[:, t] == c.pred[t]).any() for t in range(c.T))
    c.launch()
    c.check_logp()
    c.check_metrics()
    c.check_dfeat()


def test_mtl_head_single_event_labels():
    """T = 1 reading the second label column (what single_event lowers to)."""
    c = MtlCase(1, 4, 7, 64, [2], seed=111, lab_stride=2, lab_off=1)
    assert c.min_margin() > 0.5
    assert (c.lab[:, 0] == c.pred[0]).any() and (c.lab[:, 0] != c.pred[0]).any()
    c.launch()
    c.check_logp()
    c.check_metrics()
    c.check_dfeat()


@pytest.mark.parametrize("shape", [MTL_SHAPES[1], MTL_SHAPES[2]], ids=["C64", "C256"])
def test_mtl_head_eval_writes_no_gradient(shape):
    c = MtlCase(*shape, seed=120, padded=True)
    assert c.min_margin() > 0.5
    c.launch(train=False)
    c.check_logp()
    c.check_metrics()
    assert (_np(c.dfeat.float()) == CANARY).all()


@pytest.mark.parametrize("nv", [0, 1, 4, 5])
def test_mtl_head_nvalid(nv):
    """Rows >= nvalid are padding: out of the metrics and the confusion matrix only.  logp is written for every
    row (inference slices it itself) and the gradient is the full-batch one, scaled by 1/B."""
    c = MtlCase(*MTL_SHAPES[1], seed=130, padded=True)
    assert c.B == 5 and c.min_margin() > 0.5
    c.launch(nvalid=torch.full((1,), nv, device=DEV, dtype=torch.int64))
    c.check_logp()
    c.check_metrics(nv=nv)
    assert (_np(c.metrics)[:, 2] == nv).all()
    c.check_dfeat()


def test_mtl_head_ties_predict_first_class():
    c = MtlCase(*MTL_SHAPES[1], seed=140, const=True)
    for z in c.logits:
        assert (z == z[:, :1]).all()
    assert all((p == 0).all() for p in c.pred)
    c.launch()
    c.check_logp()
    lp = _np(c.logp)
    for t, K in enumerate(c.ncls):
        assert (lp[t, :, :K] == lp[t, :, :1]).all()  # bit-equal logits on the device too
    c.check_metrics()  # correct / abs_err / confusion follow from prediction 0


def test_mtl_head_accumulates():
    c = MtlCase(*MTL_SHAPES[4], seed=150)
    assert c.min_margin() > 0.5
    c.launch()
    c.launch()
    c.check_metrics(times=2)


MTL_REJECTED = [
    # T, C, ncls
    pytest.param(1, 24, [2], id="C24"),        # does not divide 256
    pytest.param(1, 512, [16], id="C512"),
    pytest.param(1, 16, [8], id="gsz2"),
    pytest.param(1, 64, [3], id="ncls3"),
    pytest.param(5, 64, [2] * 5, id="T5"),
    pytest.param(1, 256, [32], id="ncls32"),
]


@pytest.mark.parametrize("T,C,ncls", MTL_REJECTED)
def test_mtl_head_rejects(T, C, ncls):
    """Refused on the host (no launch): every output buffer keeps its canary."""
    B, HW = 2, 3
    feat = torch.zeros(T, B * HW, C, device=DEV, dtype=torch.bfloat16)
    labels = torch.zeros(B, T, device=DEV, dtype=torch.int64)
    logp = torch.full((T, B, 16), CANARY, device=DEV)
    dfeat = torch.full((T, B * HW, C), CANARY, device=DEV, dtype=torch.bfloat16)
    metrics = torch.full((T, 4), CANARY, device=DEV)
    conf = torch.full((T, 16, 16), ICANARY, device=DEV, dtype=torch.int32)
    d = {"feat": _ptr(feat), "fgs": B * HW * C, "ldf": C, "labels": _ptr(labels), "lab_stride": T, "lab_off": 0,
         "T": T, "B": B, "HW": HW, "C": C, "ncls": ncls, "w": [1.0] * T, "logp": _ptr(logp), "dfeat": _ptr(dfeat),
         "dgs": B * HW * C, "metrics": _ptr(metrics), "confusion": _ptr(conf)}
    with pytest.raises(RuntimeError):
        _lib().mtl_head(_stream(), d)
    _sync()
    assert (_np(logp) == CANARY).all() and (_np(metrics) == CANARY).all() and (_np(conf) == ICANARY).all()
    assert (_np(dfeat.float()) == CANARY).all()


# =====================================================================================================
# B. cls_head + cls_wgrad (Model C)
# =====================================================================================================
CLS_SHAPES = [
    # B, HW, C, N
    (4, 6, 2048, 32),   # the model's own head
    (3, 1, 1000, 32),   # C < 1024: the second channel of every thread is out of range; partial last wave; HW = 1
    (3, 5, 1500, 10),   # 1024 < C < 2048; a partly filled cached class array
    (2, 3, 520, 33),    # the first N on the uncached path
    (2, 3, 520, 64),    # the largest N
]


class ClsCase:
    def __init__(self, B, HW, C, N, p_drop=0.0, seed=0, padded=False, rng_seed=0, labels=None, x=None, W=None,
                 bias=None):
        self.B, self.HW, self.C, self.N, self.p = B, HW, C, N, float(p_drop)
        g = torch.Generator().manual_seed(seed)
        x0 = (torch.randn(B, HW, C, generator=g).abs() + 0.1)
        W0 = torch.randn(N, C, generator=g) / math.sqrt(C)
        b0 = torch.randn(N, generator=g)
        l0 = torch.randint(0, N, (B,), generator=g)
        x = (x0 if x is None else x).bfloat16()
        self.W = W0 if W is None else W
        self.bias = b0 if bias is None else bias
        self.lab = (l0 if labels is None else torch.as_tensor(labels, dtype=torch.int64)).numpy()
        assert self.lab.min() >= 0 and self.lab.max() < N
        self.x64 = x.double().numpy()
        self.W64, self.b64 = self.W.double().numpy(), self.bias.double().numpy()
        self.ldx = C + 8 if padded else C
        xb = torch.full((B * HW, self.ldx), NAN if padded else 0.0, dtype=torch.bfloat16)
        xb[:, :C] = x.view(B * HW, C)
        self.xb = xb.to(DEV)
        self.Wd, self.bd = self.W.to(DEV), self.bias.to(DEV)
        self.labels = torch.from_numpy(self.lab).to(DEV)
        self.rng_seed = rng_seed
        self.reset()

    def reset(self, metrics_too=True):
        B, HW, C, N = self.B, self.HW, self.C, self.N
        self.feat = torch.full((B, C), CANARY, device=DEV)
        self.logits = torch.full((B, N), CANARY, device=DEV)
        self.dlogits = torch.full((B, N), CANARY, device=DEV)
        self.dx = torch.full((B * HW, C), CANARY, device=DEV, dtype=torch.bfloat16)
        self.dW = torch.full((N, C), CANARY, device=DEV)
        self.db = torch.full((N,), CANARY, device=DEV)
        self.seed = torch.full((1,), self.rng_seed, device=DEV, dtype=torch.int64)
        if metrics_too:
            self.metrics = torch.zeros(3, 4, device=DEV)
            self.conf = torch.zeros(2, 16, 16, device=DEV, dtype=torch.int32)

    def args(self, train=True, nvalid=None, **over):
        d = {"x": _ptr(self.xb), "ldx": self.ldx, "W": _ptr(self.Wd), "bias": _ptr(self.bd), "labels": _ptr(self.labels),
             "B": self.B, "HW": self.HW, "C": self.C, "N": self.N, "p_drop": self.p, "seed": _ptr(self.seed),
             "feat": _ptr(self.feat), "logits": _ptr(self.logits), "dlogits": _ptr(self.dlogits),
             "metrics": _ptr(self.metrics), "confusion": _ptr(self.conf)}
        if train:
            d.update({"dx": _ptr(self.dx), "dW": _ptr(self.dW), "db": _ptr(self.db)})
        if nvalid is not None:
            d["nvalid"] = _ptr(nvalid)
        d.update(over)
        return d

    def launch(self, **kw):
        _lib().cls_head(_stream(), self.args(**kw))
        _sync()

    def mask(self):
        """The kernel's own keep mask: every GAP value is strictly positive, so feat == 0 <=> dropped."""
        return _np(self.feat) != 0

    def ref_logits(self, m=None):
        gap = self.x64.mean(1)
        f = gap if m is None else gap * m / (1.0 - self.p)
        return f, f @ self.W64.T + self.b64

    def expected_metrics(self, z, nv=None, times=1):
        nv = self.B if nv is None else nv
        lab, pred = self.lab[:nv], z.argmax(-1)[:nv]
        lp = _log_softmax64(z)
        ce = -lp[np.arange(self.B), self.lab][:nv].sum()
        ld, le, pd, pe = lab % 16, lab // 16, pred % 16, pred // 16
        met = np.array([[ce, (pred == lab).sum(), nv, 0],
                        [0, (pd == ld).sum(), nv, np.abs(pd - ld).sum()],
                        [0, (pe == le).sum(), nv, 0]], dtype=np.float64)
        cm = np.stack([_confusion(ld, pd), _confusion(le, pe)])
        return met * times, cm * times

    def check_metrics(self, z, nv=None, times=1):
        met, cm = self.expected_metrics(z, nv, times)
        got = _np(self.metrics).astype(np.float64)
        e = abs(got[0, 0] - met[0, 0]) / abs(met[0, 0]) if met[0, 0] else abs(got[0, 0])
        print(f"cls_head CE sum rel err {e:.3e}")
        assert e < 1e-4, (got[0, 0], met[0, 0])
        got[0, 0] = met[0, 0]
        assert np.array_equal(got, met), (got, met)
        assert np.array_equal(_np(self.conf).astype(np.int64), cm)  # [0]: [ld][pd], [1]: [le][pe]


def _cls_cases():
    out = []
    for i, s in enumerate(CLS_SHAPES):
        ps = [0.0, 0.5] + ([0.25] if i == 0 else [])
        for p in ps:
            out.append(pytest.param(s, p, False, 200 + i, id=f"{'x'.join(map(str, s))}-p{p}"))
    out.append(pytest.param(CLS_SHAPES[2], 0.5, True, 210, id=f"{'x'.join(map(str, CLS_SHAPES[2]))}-p0.5-ldx"))
    return out


@pytest.mark.parametrize("shape,p,padded,seed", _cls_cases())
def test_cls_head_reference(shape, p, padded, seed):
    B, HW, C, N = shape
    c = ClsCase(*shape, p_drop=p, seed=seed, padded=padded, rng_seed=(5 << 32) | 3)
    c.launch()
    m = c.mask()
    if p == 0.0:
        assert m.all()
    f_ref, z_ref = c.ref_logits(m)
    feat = _np(c.feat).astype(np.float64)
    e_feat = float((np.abs(feat - f_ref) / np.where(m, f_ref, 1.0)).max())
    assert e_feat < 1e-5, e_feat
    z = _np(c.logits).astype(np.float64)
    e_z = rel64(z, z_ref)
    assert e_z < 1e-4, e_z
    sm = np.exp(_log_softmax64(z_ref))
    sm[np.arange(B), c.lab] -= 1.0
    dl_ref = sm / B
    dl = _np(c.dlogits).astype(np.float64)
    e_dl = float((np.abs(dl - dl_ref) / (1e-6 + 1e-4 * np.abs(dl_ref))).max())  # <= 1 within atol 1e-6 + rtol 1e-4
    print(f"cls_head dlogits max abs err {np.abs(dl - dl_ref).max():.3e}")
    assert e_dl <= 1.0, e_dl
    dx_ref = (dl_ref @ c.W64) * m / (1.0 - p) / HW
    dxb = c.dx.view(B, HW, C)
    dx = _np(dxb.float()).astype(np.float64)
    e_dx = rel64(dx, np.broadcast_to(dx_ref[:, None, :], dx.shape))
    assert e_dx < 4e-3, e_dx  # one bf16 rounding
    bits = _bits(dxb)
    assert (bits == bits[:, :1]).all(), "dx differs between the pixels of one sample"
    assert (dx[:, 0][~m] == 0).all(), "dx is not zero on a dropped channel"
    # cls_wgrad from the head's own dlogits and features
    e_dw = rel64(_np(c.dW), dl.T @ feat)
    e_db = rel64(_np(c.db), dl.sum(0))
    assert e_dw < 1e-4 and e_db < 1e-4, (e_dw, e_db)
    print(f"cls_head rel err: feat {e_feat:.3e} logits {e_z:.3e} dx {e_dx:.3e} dW {e_dw:.3e} db {e_db:.3e}")
    assert int(c.seed.item()) == c.rng_seed + 1  # the training launch advances the dropout counter by one
    assert _np(c.metrics)[0, 2] == B


def test_cls_head_eval_writes_no_gradient():
    c = ClsCase(*CLS_SHAPES[0], p_drop=0.0, seed=220, rng_seed=41)
    c.launch(train=False)
    f_ref, z_ref = c.ref_logits(c.mask())
    assert c.mask().all()
    assert rel64(_np(c.logits), z_ref) < 1e-4
    assert int(c.seed.item()) == 41
    assert (_np(c.dW) == CANARY).all() and (_np(c.db) == CANARY).all() and (_np(c.dx.float()) == CANARY).all()


CLS_BC = [(4, 2048), (3, 1000), (3, 1500), (2, 520)]  # the distinct (B, C) of CLS_SHAPES
MASK_SEEDS = [0, 1, 2, 7, (5 << 32) | 3]


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("B,C", CLS_BC)
def test_cls_head_dropout_mask_statistics(B, C, p):
    """Binomial 5-sigma bounds (derived, not measured): the dropped fraction; two samples of one launch, the next
    training step, and another RNG stream (the counter's high word) each draw an independent mask; the same
    counter draws the same mask."""
    c = ClsCase(B, 1, C, 4, p_drop=p, seed=230)
    n = B * C
    q = 2 * p * (1 - p)

    def draw(s):
        c.rng_seed = s
        c.reset()
        c.launch(train=False)
        assert int(c.seed.item()) == s
        return c.mask()

    for s in MASK_SEEDS:
        m = draw(s)
        assert np.array_equal(m, draw(s)), "the same counter must draw the same mask"
        dropped = 1.0 - m.mean()
        assert abs(dropped - p) <= 5 * math.sqrt(p * (1 - p) / n), (s, dropped)
        rows = (m[0] != m[1]).mean()
        assert abs(rows - q) <= 5 * math.sqrt(q * (1 - q) / C), (s, rows)
        for other in (s + 1, s + 2 ** 32):
            d = (m != draw(other)).mean()
            assert abs(d - q) <= 5 * math.sqrt(q * (1 - q) / n), (s, other, d)


# joint label j = 16 * event + distance; the inputs steer sample b to class CLS_TARGET[b]
CLS_TARGET = [3, 16 + 9, 15, 16, 5, 16 + 12, 16 + 7, 2]
#            four right            ld > pd, le > pe   ld < pd, le < pe   event only wrong   distance only wrong
CLS_LABELS = [3, 16 + 9, 15, 16,   16 + 9,            4,                 7,                 11]


def _cls_metric_case(W=None, bias=None):
    B, HW, C, N = 8, 3, 520, 32
    g = torch.Generator().manual_seed(240)
    W0 = torch.randn(N, C, generator=g) / math.sqrt(C)
    b0 = torch.randn(N, generator=g)
    x = torch.randn(B, HW, C, generator=g).abs() + 0.1
    for b, j in enumerate(CLS_TARGET):
        # more weight on the channels the target class likes: just enough for a margin of 1, so that every
        # sample's cross entropy stays O(1) (a loss of 1e-6 has no fp32 digits left after lse - logit)
        like = (W0[j] > 0).double()
        for alpha in np.arange(0.0, 6.0, 0.05):
            z = (x[b].double().mean(0) + alpha * like) @ W0.double().t() + b0.double()
            top = torch.topk(z, 2)
            if int(top.indices[0]) == j and float(top.values[0] - top.values[1]) >= 1.0:
                break
        x[b] += float(alpha) * like.float()
    return ClsCase(B, HW, C, N, seed=241, labels=CLS_LABELS, x=x, W=W0 if W is None else W,
                   bias=b0 if bias is None else bias)


def _cls_metric_preconditions(c):
    _, z = c.ref_logits()
    assert _top2_margin(z).min() >= 1e-2, f"generator seed: top-two margin {_top2_margin(z).min()}"
    pred = z.argmax(-1)
    assert np.array_equal(pred, CLS_TARGET)
    ld, le, pd, pe = c.lab % 16, c.lab // 16, pred % 16, pred // 16
    assert (pred == c.lab).sum() == c.B // 2
    assert (ld < pd).any() and (ld > pd).any() and (le < pe).any() and (le > pe).any()
    return z


def test_cls_head_metrics_joint_decode():
    c = _cls_metric_case()
    z = _cls_metric_preconditions(c)
    c.launch()
    assert rel64(_np(c.logits), z) < 1e-4
    c.check_metrics(z)
    c.launch()  # a second launch accumulates
    c.check_metrics(z, times=2)


@pytest.mark.parametrize("nv", [0, 1, 7, 8])
def test_cls_head_nvalid(nv):
    c = _cls_metric_case()
    z = _cls_metric_preconditions(c)
    c.launch(nvalid=torch.full((1,), nv, device=DEV, dtype=torch.int64))
    c.check_metrics(z, nv=nv)
    assert (_np(c.metrics)[:, 2] == nv).all()
    assert rel64(_np(c.logits), z) < 1e-4  # written for every row
    sm = np.exp(_log_softmax64(z))
    sm[np.arange(c.B), c.lab] -= 1.0
    assert np.allclose(_np(c.dlogits), sm / c.B, atol=1e-6, rtol=1e-4)  # the full-batch gradient, scaled by 1/B


def test_cls_head_ties_predict_first_class():
    c = _cls_metric_case(W=torch.zeros(32, 520), bias=torch.zeros(32))
    _, z = c.ref_logits()
    assert (z == 0).all()
    c.launch()
    assert (_np(c.logits) == 0).all()
    c.check_metrics(z)  # np.argmax: the first maximum, class 0


@pytest.mark.parametrize("C,N", [pytest.param(520, 65, id="N65"), pytest.param(2049, 32, id="C2049")])
def test_cls_head_rejects(C, N):
    c = ClsCase(2, 1, C, N, seed=250, labels=[0, 1])
    c.metrics.fill_(CANARY)
    c.conf.fill_(ICANARY)
    with pytest.raises(RuntimeError):
        _lib().cls_head(_stream(), c.args())
    _sync()
    for t in (c.feat, c.logits, c.dlogits, c.dW, c.db, c.metrics):
        assert (_np(t) == CANARY).all()
    assert (_np(c.dx.float()) == CANARY).all() and (_np(c.conf) == ICANARY).all()
    assert int(c.seed.item()) == c.rng_seed


# =====================================================================================================
# C. Evaluation metrics as the lowered programs wire them
# =====================================================================================================
EVAL_B = 8
EVAL_ROWS = [3, 9, 0, 14, 6, 11, 1, 8]    # distinct dataset rows of the first batches
EVAL_ROWS2 = [15, 2, 7, 12, 4]            # the batch that is accumulated on top


def _eval_setup(which):
    from mtl_das_pytorch_amd.data.synthetic import generate
    torch.manual_seed(0)
    if which == "multi_classifier":
        from mtl_das_pytorch_amd.engine.inception import InceptionProgram
        from mtl_das_pytorch_amd.models import Multi_Classifier, encode_joint
        prog = InceptionProgram(Multi_Classifier(), EVAL_B, "cuda")
        X, d, e = generate(2 * EVAL_B, seed=1, device="cuda")
        return prog, X, encode_joint(d, e), None
    from mtl_das_pytorch_amd.engine.mtl import MTLProgram
    from mtl_das_pytorch_amd.models import MTL_Net, Single_Task_Net
    model = MTL_Net() if which == "MTL" else Single_Task_Net(task=which.split("_")[1])
    prog = MTLProgram(model, EVAL_B, "cuda")
    X, d, e = generate(2 * EVAL_B, seed=1, device="cuda", backend="torch")
    cols = {"MTL": [0, 1], "single_distance": [0], "single_event": [1]}[which]
    return prog, X, torch.stack([d, e], 1), cols


def _eval_batch(prog, X, labels, rows):
    """What EngineBackend.eval_batch + StepRunner.eval_step run, phase by phase; returns the padded index."""
    k = len(rows)
    idx = torch.tensor(list(rows) + [rows[0]] * (EVAL_B - k), device="cuda")
    prog.nvalid.fill_(k)
    prog.opt["pack"].run()
    prog.arena.clear()
    prog.gather_phase(X, labels, idx).run()
    prog.fwd_eval.run()
    torch.cuda.synchronize()
    prog.nvalid.fill_(EVAL_B)
    return idx


def _eval_expected(prog, labels, idx, k, cols):
    """Host metrics from the program's own log-probabilities (Model C: logits) and the labels of rows < k."""
    out = _np(prog.logp).astype(np.float64)
    lab = _np(labels[idx])[:k]
    if cols is None:  # Model C: joint label, rows joint / distance / event
        z = out[:k]
        assert (_top2_margin(z) > 0).all(), "data seed: a valid sample has an exact tie between its top two logits"
        pred = z.argmax(-1)
        ce = -_log_softmax64(z)[np.arange(k), lab].sum()
        ld, le, pd, pe = lab % 16, lab // 16, pred % 16, pred // 16
        met = np.array([[ce, (pred == lab).sum(), k, 0], [0, (pd == ld).sum(), k, np.abs(pd - ld).sum()],
                        [0, (pe == le).sum(), k, 0]], dtype=np.float64)
        return met, np.stack([_confusion(ld, pd), _confusion(le, pe)])
    ncls = list(prog.model.task_cate_num)
    met = np.zeros((len(cols), 4))
    cm = np.zeros((len(cols), 16, 16), np.int64)
    for t, col in enumerate(cols):
        lp = out[t, :k, :ncls[t]]
        assert (_top2_margin(lp) > 0).all(), "data seed: a valid sample has an exact tie between its top two log-probabilities"
        pred, l = lp.argmax(-1), lab[:, col]
        met[t] = [-lp[np.arange(k), l].sum(), (pred == l).sum(), k, np.abs(pred - l).sum()]
        cm[t] = _confusion(l, pred)
    return met, cm


def _eval_compare(prog, met, cm):
    got = _np(prog.metrics).astype(np.float64)
    loss = met[:, 0] != 0
    assert np.allclose(got[:, 0][loss], met[:, 0][loss], rtol=1e-4, atol=0), (got, met)
    got[:, 0][loss] = met[:, 0][loss]
    assert np.array_equal(got, met), (got, met)
    assert np.array_equal(_np(prog.confusion).astype(np.int64), cm)


@pytest.mark.parametrize("which", ["MTL", "single_distance", "single_event", "multi_classifier"])
def test_eval_metrics_as_wired(which):
    """lab_off, the Model C metric rows read_metrics relies on, and the nvalid pointer: a last evaluation batch
    padded with copies of its first row must report the valid rows only."""
    prog, X, labels, cols = _eval_setup(which)
    for k in (1, 5, 8):
        prog.metrics.zero_()
        prog.confusion.zero_()
        idx = _eval_batch(prog, X, labels, EVAL_ROWS[:k])
        met, cm = _eval_expected(prog, labels, idx, k, cols)
        assert (met[:, 2] == k).all()
        _eval_compare(prog, met, cm)
        assert int(prog.nvalid.item()) == EVAL_B
    idx = _eval_batch(prog, X, labels, EVAL_ROWS2)  # not zeroed: the sum of the two batches
    met2, cm2 = _eval_expected(prog, labels, idx, len(EVAL_ROWS2), cols)
    _eval_compare(prog, met + met2, cm + cm2)
