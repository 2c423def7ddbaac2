"""fp64 reference of the fused backward join: the data gradient of a conv plus its added gradient sources, and the
backward of the BN tail that gradient feeds (plain torch on the CPU, no GPU, no project code).

The kernels evaluate the tail's BN from the fp32 constants (scale, shift, mean, invstd) the forward published;
the reference takes the same four numbers per channel, so the two sides cannot differ in the mean or the variance,
only in how they evaluate ``y * scale + shift`` (fp32 against fp64).  For the ReLU-type kinds that difference can
flip the mask of an element whose ReLU argument is within the fp32 evaluation error of zero; :func:`mask` returns
the elements within ``AMBIG`` of zero (the fp32 error is below 1e-6) so a test can bound their effect.

tests/test_bwd_ref.py checks every function here against fp64 ``torch.autograd``."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SIGMOID, SIGMUL, ADD_RELU, POOL_RELU = range(6)
AMBIG = 1e-4   # |ReLU argument| (or gap between a pool window's two largest values) below which a mask may flip
EPS = 1e-5
DEVICE = "cpu"  # where the references compute (tests/layer_ref.py ``on`` moves whole layers to the GPU)


def f64(t):
    return t.detach().to(DEVICE, torch.float64)


def join(w, dy, in_hw, stride=1, padding=0, sources=()):
    """g = dgrad(dy) + sum(sources), fp64 NHWC ``[B, H, W, Ci]``.  ``w`` [Co, Ci, KH, KW] is rounded to bf16 as the
    kernels' packed weight image is; ``dy`` NHWC [B, Ho, Wo, Co] and ``sources`` NHWC [B, H, W, Ci] are bf16."""
    w = f64(w.to(torch.bfloat16))
    s = (stride, stride) if isinstance(stride, int) else tuple(stride)
    p = (padding, padding) if isinstance(padding, int) else tuple(padding)
    Ho, Wo = dy.shape[1:3]
    op = (in_hw[0] - ((Ho - 1) * s[0] - 2 * p[0] + w.shape[2]), in_hw[1] - ((Wo - 1) * s[1] - 2 * p[1] + w.shape[3]))
    g = F.conv_transpose2d(f64(dy).permute(0, 3, 1, 2), w, None, s, p, op).permute(0, 2, 3, 1)
    for t in sources:
        g = g + f64(t)
    return g.contiguous()


def batch_consts(y, gamma, beta, eps=EPS, dtype=torch.float32):
    """[4, C] (scale, shift, mean, invstd) of the training-mode BN of NHWC ``y``, computed in fp64 and rounded to
    ``dtype``: what the forward tail publishes for the backward kernels."""
    y = f64(y)
    mean = y.mean((0, 1, 2))
    inv = 1.0 / torch.sqrt(y.var((0, 1, 2), unbiased=False) + eps)
    scale = f64(gamma) * inv
    return torch.stack([scale, f64(beta) - mean * scale, mean, inv]).to(dtype)


def up(g, H, W):
    """A gradient on the 2x2 / ceil-mode pooled grid repeated over its windows."""
    return g.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]


def mask(kind, y, consts, r=None, consts2=None, ambig=AMBIG):
    """(m, amb): dz = g * m elementwise (``g`` repeated over the pool windows for POOL_RELU) and the boolean map of
    the elements whose mask the kernels' fp32 evaluation may legitimately decide the other way (None for the kinds
    without a ReLU; ``ambig``: their distance from the decision).  ``consts2`` given: ADD_RELU with a projection shortcut, the residual is BN2(r)."""
    y, k = f64(y), f64(consts)
    t = y * k[0] + k[1]
    if kind == ACT_NONE:
        return torch.ones_like(t), None
    if kind == ACT_RELU:
        return (t > 0).double(), t.abs() < ambig
    if kind == ACT_SIGMOID:
        s = torch.sigmoid(t)
        return s * (1 - s), None
    if kind == SIGMUL:
        s = torch.sigmoid(t)
        return f64(r) * s * (1 - s), None
    if kind == ADD_RELU:
        rr = f64(r)
        if consts2 is not None:
            k2 = f64(consts2)
            rr = rr * k2[0] + k2[1]
        return (t + rr > 0).double(), (t + rr).abs() < ambig
    if kind == POOL_RELU:  # the gradient goes to the first maximum (row-major) of each window, if positive
        B, H, W, C = t.shape
        Hp, Wp = (H + 1) // 2, (W + 1) // 2
        tp = torch.full((B, 2 * Hp, 2 * Wp, C), float("-inf"), dtype=torch.float64, device=t.device)
        tp[:, :H, :W] = t
        win = tp.view(B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Hp, Wp, C, 4)
        top, am = win.max(-1), win.argmax(-1)
        top = top.values
        sel = F.one_hot(am, 4).double() * (top > 0).double().unsqueeze(-1)
        second = win.masked_fill(F.one_hot(am, 4).bool(), float("-inf")).max(-1).values
        close = (top.abs() < ambig) | ((top > 0) & (top - second < ambig) & (top != second))
        ambw = close.unsqueeze(-1) & (win >= (top - ambig).unsqueeze(-1))

        def back(v):
            return v.view(B, Hp, Wp, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Hp, 2 * Wp, C)[:, :H, :W]
        return back(sel).contiguous(), back(ambw).contiguous()
    raise ValueError(kind)


def tail(kind, y, consts, gamma, g, r=None, consts2=None, gamma2=None, gscale=1.0):
    """Backward of the tail ``act(BN(y))`` for the gradient ``g`` (a tensor or a list of sources, summed in fp64).
    Returns a dict: ``dz``; ``amb``; ``sdz`` = sum(dz), ``sdzx`` = sum(dz * xhat), ``sdzx2`` = sum(dz * xhat2)
    (projection) per channel; ``dy``, ``dy2`` (projection), ``side`` (SIGMUL: the multiplier's gradient, ADD_RELU
    identity: the shortcut's); ``dgamma``, ``dbeta`` (and ``dgamma2``, ``dbeta2``) scaled by ``gscale``."""
    y, k = f64(y), f64(consts)
    if isinstance(g, (list, tuple)):
        g = sum(f64(t) for t in g)
    g = f64(g)
    B, H, W, C = y.shape
    n = B * H * W
    if kind == POOL_RELU:
        g = up(g, H, W)
    m, amb = mask(kind, y, consts, r, consts2)
    dz = g * m
    xh = (y - k[2]) * k[3]
    o = {"dz": dz, "amb": amb, "xhat": xh, "sdz": dz.sum((0, 1, 2)), "sdzx": (dz * xh).sum((0, 1, 2))}
    o["dy"] = f64(gamma) * k[3] * (dz - o["sdz"] / n - xh * o["sdzx"] / n)
    o["dgamma"], o["dbeta"] = o["sdzx"] * gscale, o["sdz"] * gscale
    o["side"] = o["dy2"] = None
    if kind == SIGMUL:
        o["side"] = g * torch.sigmoid(y * k[0] + k[1])
    elif kind == ADD_RELU and consts2 is None:
        o["side"] = dz
    elif kind == ADD_RELU:
        k2 = f64(consts2)
        xh2 = (f64(r) - k2[2]) * k2[3]
        o["xhat2"], o["sdzx2"] = xh2, (dz * xh2).sum((0, 1, 2))
        o["dy2"] = f64(gamma2) * k2[3] * (dz - o["sdz"] / n - xh2 * o["sdzx2"] / n)
        o["dgamma2"], o["dbeta2"] = o["sdzx2"] * gscale, o["sdz"] * gscale
    return o


# ---------------------------------------------------------------------------------------------------
# Inputs of the GPU tests (tests/test_bwd_join_gpu.py); tests/test_bwd_ref.py asserts their ambiguous share.
def tail_inputs(seed, B, H, W, C):
    """bf16 y ~ 2 N(0,1) + 0.3, r ~ N(0,1), y2 ~ N(0,1) + 1 (NHWC), fp32 BN parameters and batch constants of y
    (``k``) and of y2 (``k2``, the projection shortcut's BN)."""
    gen = torch.Generator().manual_seed(seed)
    d = {"y": (2 * torch.randn(B, H, W, C, generator=gen) + 0.3).bfloat16(),
         "r": torch.randn(B, H, W, C, generator=gen).bfloat16(),
         "y2": (torch.randn(B, H, W, C, generator=gen) + 1).bfloat16(),
         "gamma": torch.rand(C, generator=gen) + 0.5, "beta": 0.1 * torch.randn(C, generator=gen),
         "gamma2": torch.rand(C, generator=gen) + 0.5, "beta2": 0.1 * torch.randn(C, generator=gen)}
    d["k"] = batch_consts(d["y"], d["gamma"], d["beta"])
    d["k2"] = batch_consts(d["y2"], d["gamma2"], d["beta2"])
    return d


# the kinds of the tests as (kernel kind, projection shortcut)
KINDS = {"none": (ACT_NONE, False), "relu": (ACT_RELU, False), "sigmoid": (ACT_SIGMOID, False),
         "sigmul": (SIGMUL, False), "add": (ADD_RELU, False), "add_proj": (ADD_RELU, True), "pool": (POOL_RELU, False)}


def kind_mask(name, t, ambig=AMBIG):
    """:func:`mask` of a named kind on :func:`tail_inputs`."""
    kind, proj = KINDS[name]
    r = t["y2"] if proj else (t["r"] if kind in (SIGMUL, ADD_RELU) else None)
    return mask(kind, t["y"], t["k"], r, t["k2"] if proj else None, ambig)


def kind_tail(name, t, g, gscale=1.0):
    """:func:`tail` of a named kind on :func:`tail_inputs`."""
    kind, proj = KINDS[name]
    r = t["y2"] if proj else (t["r"] if kind in (SIGMUL, ADD_RELU) else None)
    return tail(kind, t["y"], t["k"], t["gamma"], g, r, t["k2"] if proj else None, t["gamma2"] if proj else None, gscale)


BASE = (2, 17, 42)           # B, H, W of the join tests: 1428 pixels
JOIN_SEEDS = (3, 7)          # tail inputs of the dgrad-epilogue tests (C = 32): group 0 / group 1
JOIN_MARGIN = 1e-5           # no ReLU argument of theirs is closer to zero: 10 x the kernels' fp32 evaluation error,
                             # so every mask is decided and d(gamma), d(beta) can be held to 1e-5
JOIN_KINDS = ("relu", "add", "add_proj")
# BN tail backward modes: (seed, B, H, W, C, kinds)
RELU_KINDS = ("relu", "add", "add_proj", "pool")
TAIL_INPUTS = ([(10 + i, 2, 17, 42, C, tuple(KINDS)) for i, C in enumerate((8, 48, 128))] +   # sources, subset reduce
               [(20, 2, 17, 42, 48, tuple(KINDS)), (21, 2, 17, 42, 48, tuple(KINDS))] +       # the two groups
               [(30, 2, 16, 32, 8, tuple(KINDS)), (31, 2, 32, 32, 8, tuple(KINDS)),           # single launch R = 1, 2,
                (32, 4, 32, 32, 8, tuple(k for k in KINDS if not k.startswith("add")))] +     # 4 (not the residual kinds)
               [(40, 2, 17, 41, 48, ("pool",))])                                              # odd H and W
