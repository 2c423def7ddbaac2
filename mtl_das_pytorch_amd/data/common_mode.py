"""Common-mode removal ahead of the windows: the part of a DAS recording that is the same on every fiber position at
a time sample -- laser phase noise, vibration of the interrogator itself -- estimated per sample and subtracted.

This module is the definition (numpy) that every layer is tested against; csrc/common_mode.hip evaluates it on the
device, bit for bit.  For ``x`` [C, F, T] fp32 and ``how`` in ``("median", "mean")``

    y[c, f, t] = fp32(x[c, f, t] - m[c, t])        one IEEE fp32 subtraction

``"median"``: ``m[c, t] = sorted(x[c, :, t])[(F - 1) // 2]``, the lower median over the fiber, NaN sorted after every
number (as ``np.sort`` does; the convention of ``inference.running_floor_reference``) and a median that is a zero of
either sign taken as ``+0.0``.  It is an element of its column, hence exact.  A column with more than half NaN has a
NaN median and becomes NaN; with fewer the median is finite and only the NaN samples stay NaN.

``"mean"``: ``acc = 0.0`` in fp64, ``acc += x[c, f, t]`` for ``f = 0 .. F - 1`` in that order, ``m = fp32(acc / F)``.
The order is part of the definition (``np.sum`` adds pairwise and is not it): the same additions in the same order
give the same bits anywhere.

Every time column is independent of every other, so a stream has the same bits however it is cut and carries no
state.  The mean commutes with a FIR along time (both are linear); the median does not.

Not offered: an estimate over a sub-range of the fiber only.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

HOWS = ("median", "mean")


def as_common_mode(arg) -> Optional[str]:
    """The checked ``common_mode`` argument: None (off), ``"median"`` or ``"mean"``; ``ValueError`` otherwise."""
    if arg is None:
        return None
    if not isinstance(arg, str) or arg not in HOWS:
        raise ValueError(f"common_mode must be None, 'median' or 'mean', got {arg!r}")
    return arg


def common_mode_reference(x, how) -> Tuple[np.ndarray, np.ndarray]:
    """``(y, m)`` of the definition above: ``y`` fp32 like ``x`` ([C, F, T]; [F, T] is one channel), ``m`` fp32
    [C, T], the value subtracted."""
    how = as_common_mode(how)
    if how is None:
        raise ValueError("common_mode_reference needs 'median' or 'mean'")
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[1] < 1:
        raise ValueError(f"a recording is [F, T] or [C, F, T] with F >= 1, got {x.shape}")
    C, Fn, T = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if how == "median":
            m = np.sort(x, axis=1)[:, (Fn - 1) // 2, :]
            m = np.where(m == 0, np.float32(0.0), m)  # -0.0 == 0: a zero of either sign becomes +0.0
        else:
            acc = np.zeros((C, T), dtype=np.float64)
            for f in range(Fn):
                acc += x[:, f, :]
            m = (acc / Fn).astype(np.float32)
        y = x - m[:, None, :]
    return y.astype(np.float32, copy=False), m.astype(np.float32, copy=False)
