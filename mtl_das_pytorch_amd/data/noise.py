"""SNR noise of the batch gather, defined once in numpy fp64.

This module is the definition: the HIP kernels (csrc/augment.hip) evaluate it in fp32 and are tested against it, and
the plain-PyTorch backend calls it directly.  For dataset row ``s``, channel ``c``, pixel ``(h, w)`` of an
``[N, C, H, W]`` fp32 set, a 64-bit ``seed``, a draw number ``draw`` and a stream id ``k``:

  power     P[s, c] = mean over H*W of (x - mean(x))^2 of the clean plane (add_gaussian's signal-power estimator)
  gaussian  g(s, c, h, w) = BM(philox(ctr, key))[h & 3] with
              ctr = ((h >> 2) * W + w,  c | (k << 8),  s mod 2^32,  draw mod 2^32),   key = (seed_lo, seed_hi)
            BM: u01(x) = ((x >> 8) + 1) * 2^-24; words (x, y) give m0 cos, m0 sin; words (z, w) give m1 cos, m1 sin
            (m = sqrt(-2 ln u01(first)), angle = 2 pi u01(second)) -- the Box-Muller of csrc/synth.hip
  level     training: snr_s = lo + (hi - lo) * u01(philox((0, 1 << 8, s, draw), key).x), shared by the sample's
            channels; evaluation: the fixed level it is given
  value     y = x + sigma * g,  sigma[s, c] = sqrt(P[s, c] * 10^(-snr / 10))

One Philox call serves a vertical quad of pixels (rows 4q .. 4q + 3 of one column): the stem's tap packing needs
consecutive rows of a column.  Stream ids: 0 the training Gaussian, 1 the training SNR draw, 2 the evaluation
Gaussian.  Unlike the reference's ``add_gaussian`` the noise is not rescaled by its own sample standard deviation,
so the SNR holds in expectation (docs/PARITY.md R21).  The noise depends on (seed, draw, dataset row, c, h, w)
only: not on the batch position, the launch geometry, the rank or the world size.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

STREAM_TRAIN, STREAM_SNR, STREAM_EVAL = 0, 1, 2
# evaluation noise is the same for every model and run (as tools/accuracy_table.py's fixed seeds)
EVAL_SEED = 0x5EEDDA5
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox_np(ctr: np.ndarray, key: int) -> np.ndarray:
    """Philox-4x32-10 on uint32 counters [n, 4] (Salmon et al., SC'11), vectorised in NumPy."""
    c = ctr.astype(np.uint64)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[:, 0]
        p1 = np.uint64(M1) * c[:, 2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = np.stack([hi1 ^ c[:, 1] ^ k0, lo1, hi0 ^ c[:, 3] ^ k1, lo0], 1)
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return c.astype(np.uint32)


def u01(x: np.ndarray) -> np.ndarray:
    """Uniform in (0, 1] from a 32-bit word (exact in fp32 and fp64)."""
    return ((x >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def parse_snr_range(v) -> Optional[Tuple[float, float]]:
    """``"LO[,HI]"`` / a number / a pair -> (lo, hi); None stays None.  One value means lo == hi."""
    if v is None:
        return None
    if isinstance(v, str):
        v = [float(t) for t in v.split(",") if t.strip() != ""]
    elif np.isscalar(v):
        v = [float(v)]
    v = [float(t) for t in v]
    if len(v) == 1:
        v = v * 2
    if len(v) != 2 or not all(np.isfinite(v)) or v[0] > v[1]:
        raise ValueError(f"SNR range must be LO or LO,HI with LO <= HI, got {v}")
    return v[0], v[1]


def sample_power(X: np.ndarray) -> np.ndarray:
    """[N, C, H, W] -> P [N, C] (fp64): the plane's mean squared deviation from its mean."""
    x = np.asarray(X, dtype=np.float64)
    return ((x - x.mean((2, 3), keepdims=True)) ** 2).mean((2, 3))


def gaussian(rows: Sequence[int], C: int, H: int, W: int, seed: int, draw: int, stream: int) -> np.ndarray:
    """g [len(rows), C, H, W] (fp64) of the dataset rows ``rows``."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n, nq = len(rows), (H + 3) // 4
    s, c, q, w = np.meshgrid(rows, np.arange(C), np.arange(nq), np.arange(W), indexing="ij")
    ctr = np.stack([q * W + w, c | (stream << 8), s % 2 ** 32, np.full_like(s, draw % 2 ** 32)], -1)
    r = philox_np(ctr.reshape(-1, 4).astype(np.uint64).astype(np.uint32), seed).reshape(n, C, nq, W, 4)
    m0, m1 = np.sqrt(-2.0 * np.log(u01(r[..., 0]))), np.sqrt(-2.0 * np.log(u01(r[..., 2])))
    a0, a1 = 2.0 * np.pi * u01(r[..., 1]), 2.0 * np.pi * u01(r[..., 3])
    quad = np.stack([m0 * np.cos(a0), m0 * np.sin(a0), m1 * np.cos(a1), m1 * np.sin(a1)], 3)  # [n, C, nq, 4, W]
    return quad.reshape(n, C, nq * 4, W)[:, :, :H]


def sample_snr(rows: Sequence[int], lo: float, hi: float, seed: int, draw: int) -> np.ndarray:
    """The training level of each dataset row at ``draw`` (fp64 [len(rows)]), uniform in (lo, hi]."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    ctr = np.zeros((len(rows), 4), dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = 1 << 8, rows % 2 ** 32, draw % 2 ** 32
    return lo + (hi - lo) * u01(philox_np(ctr.astype(np.uint32), seed)[:, 0])


def sigma(P: np.ndarray, snr_db) -> np.ndarray:
    """sigma [n, C] from the power rows P [n, C] and a level (a scalar, or one per row)."""
    snr = np.asarray(snr_db, dtype=np.float64).reshape(-1, 1)
    return np.sqrt(np.asarray(P, dtype=np.float64) * 10.0 ** (-snr / 10.0))


def add_noise(X: np.ndarray, rows: Sequence[int], seed: int, draw: int, snr: Tuple[float, float] = None,
              snr_db: float = None, power: np.ndarray = None, stream: Optional[int] = None) -> np.ndarray:
    """The noisy rows ``rows`` of the clean set ``X`` [N, C, H, W], fp64 [len(rows), C, H, W].

    ``snr = (lo, hi)``: the training form (Gaussian stream 0, per-sample level from stream 1).  ``snr_db``: the
    evaluation form (Gaussian stream 2, that level).  ``power``: P of the whole set (sample_power(X)) when the
    caller has it already; ``stream`` overrides the Gaussian's stream id."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    P = None if power is None else np.asarray(power, dtype=np.float64)[rows]
    return noisy_rows(np.asarray(X)[rows], rows, seed, draw, snr=snr, snr_db=snr_db, power=P, stream=stream)


def noisy_rows(x: np.ndarray, rows: Sequence[int], seed: int, draw: int, snr: Tuple[float, float] = None,
               snr_db: float = None, power: np.ndarray = None, stream: Optional[int] = None) -> np.ndarray:
    """:func:`add_noise` of rows already gathered: ``x`` [n, C, H, W] are the clean dataset rows ``rows`` (and
    ``power`` [n, C] theirs)."""
    if (snr is None) == (snr_db is None):
        raise ValueError("exactly one of snr=(lo, hi) / snr_db")
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    x = np.asarray(x).astype(np.float64)
    P = sample_power(x) if power is None else np.asarray(power, dtype=np.float64)
    if snr is not None:
        level = sample_snr(rows, float(snr[0]), float(snr[1]), seed, draw)
        k = STREAM_TRAIN if stream is None else stream
    else:
        level = float(snr_db)
        k = STREAM_EVAL if stream is None else stream
    g = gaussian(rows, x.shape[1], x.shape[2], x.shape[3], seed, draw, k)
    return x + sigma(P, level)[:, :, None, None] * g
