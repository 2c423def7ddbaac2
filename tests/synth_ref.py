"""fp64 reference of the on-device synthetic generator (csrc/synth.hip; tests/test_synth.py): the physical model of
data/synthetic.py evaluated in fp64 from the fp32 per-sample parameters (the nine values of a ``params`` row) and the
fp32 ``torch.linspace`` axes widened to fp64, and the generator's Gaussian plane from data/noise.py's Philox and u01.

Layout of the noise: element e = h W + w of channel c of global sample sample0 + s takes normal e % 4 of the Philox
call with counter (e // 4, c, (sample0 + s) mod 2^32, 0) and key words (low, high); the four normals are m0 cos, m0 sin
(words x, y) and m1 cos, m1 sin (words z, w).  Channel c is the clean plane rolled by c mod W along the time axis.
numpy / CPU torch only; nothing here imports the extension.
"""
import math

import numpy as np
import torch

from mtl_das_pytorch_amd.data.noise import philox_np, u01

AMBIGUOUS_TAU = 2e-6     # |tau| (or its distance from a multiple of the period) below which fp32 and fp64 may pick
                         # different branches of the step / the remainder
AMBIGUOUS_CAP = 1e-4     # share of a case's elements that may be ambiguous

# (H, W, C, n): 35 and 63 elements end in a partial Philox quad; a single row; a single column (linspace of one
# point); C > 1 with W = 2 (the roll's c % W); the models' map
CASES = [(5, 7, 1, 3), (5, 7, 3, 3), (9, 7, 3, 3), (1, 9, 1, 3), (13, 1, 3, 3), (4, 2, 3, 3), (100, 250, 1, 8),
         (100, 250, 3, 8)]
KEYS = [0x2545F491, 0x123456789ABCDEF0]   # below 2^31; a non-zero high word (below 2^63)
SAMPLE0 = [0, 5]


def case_id(c):
    return f"{c[0]}x{c[1]}_C{c[2]}"


def params(n, seed):
    """The [n, 9] fp32 parameter rows of ``generate(n, seed, distance=..., event=...)`` (the same CPU draws in the
    same order) and the labels: both event types and distances 0 and 15 are forced into rows 0 and 1."""
    g = torch.Generator().manual_seed(1000 + seed)
    distance = torch.randint(0, 16, (n,), generator=g)
    event = torch.randint(0, 2, (n,), generator=g)
    distance[0], distance[1], event[0], event[1] = 0, 15, 0, 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    x0 = torch.rand(n, generator=g) * 0.5 + 0.25
    t0 = torch.rand(n, generator=g) * 0.35 + 0.1
    jitter = torch.rand(n, 4, generator=g)
    snr = torch.rand(n, generator=g) * 14.0 + 6.0
    p = torch.cat([distance.float().view(n, 1), event.float().view(n, 1), x0.view(n, 1), t0.view(n, 1),
                   jitter.view(n, 4), snr.view(n, 1)], 1).contiguous()
    return p, distance, event


def model(p, H, W):
    """The clean plane of every row of ``p`` [n, 9] (fp32) in fp64: dict of ``clean``, ``env`` (amp x footprint: the
    bound of |clean|), ``tau``, ``ambiguous`` [n, H, W], ``p_sig`` and ``sigma`` [n]."""
    q = p.double().numpy()
    n = q.shape[0]
    col = lambda i: q[:, i].reshape(n, 1, 1)  # noqa: E731
    xs = torch.linspace(0, 1, H).double().numpy().reshape(1, H, 1)
    ts = torch.linspace(0, 1, W).double().numpy().reshape(1, 1, W)
    dist_m, ev = col(0) + 0.5, col(1)
    dx = (xs - col(2)) * 20.0
    tau = ts - (col(3) + np.sqrt(dist_m ** 2 + dx ** 2) / 110.0)
    footprint = np.exp(-(dx ** 2) / (2.0 * (1.5 + 0.6 * dist_m) ** 2))
    amp = 1.0 / (1.0 + dist_m / 4.0)
    f_strike, period = 38.0 + 6.0 * col(4), 0.16 + 0.04 * col(5)
    phase = np.mod(tau, period)   # the sign of the divisor, as torch.remainder
    strike = np.exp(-phase / 0.012) * np.cos(2 * math.pi * f_strike * phase) * (tau > 0)
    f_dig = 9.0 + 3.0 * col(6)
    dig = np.exp(-((tau - 0.18) ** 2) / (2 * 0.09 ** 2)) * np.sin(2 * math.pi * f_dig * tau + 6.28 * col(7))
    env = amp * footprint * np.ones_like(tau)
    clean = env * ((1 - ev) * strike + ev * dig)
    near_period = np.abs(tau - np.round(tau / period) * period) < AMBIGUOUS_TAU
    ambiguous = (np.abs(tau) < AMBIGUOUS_TAU) | (near_period & (ev == 0))
    p_sig = np.maximum((clean ** 2).mean((1, 2)), 1e-12)
    sigma = np.sqrt(p_sig / 10.0 ** (q[:, 8] / 10.0))
    return {"clean": clean, "env": env, "tau": tau, "ambiguous": ambiguous, "p_sig": p_sig, "sigma": sigma}


def rolled(a, C):
    """[n, H, W] -> [n, C, H, W]: channel c is the plane rolled by c mod W along the last axis (torch.roll's
    direction: out[..., w] = a[..., (w - c) mod W])."""
    W = a.shape[-1]
    return np.stack([np.roll(a, c % W, axis=-1) for c in range(C)], 1)


def gaussian(n, C, H, W, key, sample0):
    """g [n, C, H, W] (fp64) in the generator's layout."""
    nq = (H * W + 3) // 4
    s, c, qd = np.meshgrid(np.arange(n), np.arange(C), np.arange(nq), indexing="ij")
    ctr = np.stack([qd, c, (s + sample0) % 2 ** 32, np.zeros_like(s)], -1).reshape(-1, 4)
    r = philox_np(ctr.astype(np.uint64).astype(np.uint32), key).reshape(n, C, nq, 4)
    m0, m1 = np.sqrt(-2.0 * np.log(u01(r[..., 0]))), np.sqrt(-2.0 * np.log(u01(r[..., 2])))
    a0, a1 = 2.0 * np.pi * u01(r[..., 1]), 2.0 * np.pi * u01(r[..., 3])
    quad = np.stack([m0 * np.cos(a0), m0 * np.sin(a0), m1 * np.cos(a1), m1 * np.sin(a1)], -1)  # [n, C, nq, 4]
    return quad.reshape(n, C, nq * 4)[:, :, :H * W].reshape(n, C, H, W)


def reference(p, C, H, W, key=0, sample0=0):
    """Everything the tests compare, per channel [n, C, H, W]: ``clean``, ``env``, ``ambiguous``, ``g``; ``sigma``
    [n, 1, 1, 1]; ``noisy`` = clean + sigma g.  (The generator stores 100 x these.)"""
    m = model(p, H, W)
    n = p.shape[0]
    out = {k: rolled(m[k], C) for k in ("clean", "env", "ambiguous")}
    out["sigma"] = m["sigma"].reshape(n, 1, 1, 1)
    out["g"] = gaussian(n, C, H, W, key, sample0)
    out["noisy"] = out["clean"] + out["sigma"] * out["g"]
    return out
