"""Raw-rate recordings: an anti-alias FIR and decimation by an integer factor ahead of the windows.

The models take recordings at their own sample rate; an interrogator delivers a multiple of it.  This module is the
definition (numpy fp64) that every layer is tested against -- csrc/resample.hip evaluates it on the device -- and
the host's integer bookkeeping of a stream that is decimated piece by piece.

With the raw stream ``x[.., t]``, ``t = 0 .. T - 1``, the taps ``h[0 .. L - 1]`` and the factor ``D >= 1``

    y[.., k] = sum_{i = 0}^{L - 1} h[i] x[.., k D + (L - 1) - i]        k = 0 .. K - 1
    K = (T - L) // D + 1  if T >= L, else 0

the "valid" form: an output exists only when its whole support ``[k D, k D + L - 1]`` lies inside the stream (no
zero-padded edge, no look-ahead), ``np.convolve(x, h, "valid")[::D]``.  Output ``k`` becomes available when raw
sample ``k D + L - 1`` has arrived; raw samples at the end of a stream that complete no output are dropped.
``h = [1]`` is plain subsampling, ``h = ones(D) / D`` the block mean, ``D = 1`` a causal FIR.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

MAX_FACTOR = 64   # 1 <= D <= MAX_FACTOR
MAX_TAPS = 1025   # 1 <= L <= MAX_TAPS
KAISER_BETA = 6.0  # the default taps' window


def check_decimation(D, L: int) -> Tuple[int, int]:
    """``(D, L)`` as ints, inside the limits the device kernel serves; ``ValueError`` otherwise."""
    if isinstance(D, bool) or int(D) != D:
        raise ValueError(f"the decimation factor must be an integer, got {D!r}")
    D, L = int(D), int(L)
    if not 1 <= D <= MAX_FACTOR:
        raise ValueError(f"1 <= D <= {MAX_FACTOR}, got D = {D}")
    if not 1 <= L <= MAX_TAPS:
        raise ValueError(f"1 <= L <= {MAX_TAPS} taps, got L = {L}")
    return D, L


def output_count(T: int, L: int, D: int) -> int:
    """K of the definition."""
    return (T - L) // D + 1 if T >= L else 0


def decimation_taps(D: int) -> np.ndarray:
    """The default anti-alias filter of factor ``D``, fp64 [16 D + 1]: a Kaiser-windowed (``beta = 6``) sinc with
    its cut-off at ``0.375 / D`` cycles per raw sample, divided by its sum (unity at DC).  At most -52 dB at and
    above the new Nyquist ``0.5 / D`` (-61.9 dB measured) and within 0.01 dB of unity up to ``0.25 / D`` (0.0078 dB).
    A Hamming window, at the same length and cut-off, reaches the first (-52.0 dB) but not the second: its own
    pass-band ripple, all on one side once DC is pinned to unity, is 0.034 .. 0.039 dB.  ``D = 1``: ``[1.0]``."""
    D, _ = check_decimation(D, 1)
    if D == 1:
        return np.ones(1)
    L = 16 * D + 1
    n = np.arange(L) - (L - 1) / 2
    fc = 0.375 / D
    h = 2 * fc * np.sinc(2 * fc * n) * np.kaiser(L, KAISER_BETA)
    return h / h.sum()


def as_taps(taps, D: int) -> np.ndarray:
    """The taps a decimation by ``D`` runs with, fp32 [L]: ``taps`` (None: :func:`decimation_taps`) rounded to
    fp32, the values the kernel multiplies by and the fp64 reference is given."""
    h = decimation_taps(D) if taps is None else np.asarray(taps, dtype=np.float64)
    if h.ndim != 1:
        raise ValueError(f"taps must be a vector, got shape {h.shape}")
    check_decimation(D, len(h))
    return h.astype(np.float32)


def fir_decimate_reference(x, taps, D: int) -> np.ndarray:
    """The definition: fp64 ``[.., K]`` of ``x`` ``[.., T]`` (any leading dimensions).  A sum over the taps in the
    order ``i = 0 .. L - 1``, the same fp64 operations for an output wherever its support lies in ``x`` -- so a
    stream decimated piece by piece (:class:`HostDecimator`) has the bits of the stream decimated at once."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(taps, dtype=np.float64)
    if h.ndim != 1 or len(h) < 1 or int(D) < 1:
        raise ValueError("taps must be a non-empty vector and D positive")
    L, D, T = len(h), int(D), x.shape[-1]
    K = output_count(T, L, D)
    y = np.zeros(x.shape[:-1] + (K,))
    if K == 0:
        return y
    for i in range(L):
        j = L - 1 - i
        y += h[i] * x[..., j:j + (K - 1) * D + 1:D]
    return y


class DecimatorBook:
    """The host's integer mirror of a decimated stream, in the style of ``inference.LiveBook``: ``raw_total`` raw
    samples received, ``k_next`` outputs produced.  Between pushes the stream carries the raw samples from the next
    output's support on, ``carry_len = max(0, raw_total - k_next D) <= L - 1`` of them, or -- only when ``D > L`` --
    the support starts ``skip = max(0, k_next D - raw_total)`` samples into what has not arrived yet.  The device is
    never read."""

    def __init__(self, L: int, D: int):
        self.D, self.L = check_decimation(D, L)
        self.raw_total = 0
        self.k_next = 0

    @property
    def carry_len(self) -> int:
        return max(0, self.raw_total - self.k_next * self.D)

    @property
    def skip(self) -> int:
        return max(0, self.k_next * self.D - self.raw_total)

    def push(self, n: int) -> Tuple[int, int, int]:
        """``n`` more raw samples: ``(m, carry_len, skip)`` -- the outputs ``k_next .. k_next + m - 1`` the push
        yields and the carry and skip it starts from, the arguments of its ``fir_decimate`` launch."""
        n = int(n)
        if n < 0:
            raise ValueError(f"a push of {n} samples")
        carry_len, skip = self.carry_len, self.skip
        self.raw_total += n
        m = output_count(self.raw_total, self.L, self.D) - self.k_next
        self.k_next += m
        return m, carry_len, skip

    def plan(self, sizes) -> List[Tuple[int, int, int]]:
        """What :meth:`push` would return for pushes of ``sizes`` in turn; the book stays as it is."""
        state = (self.raw_total, self.k_next)
        try:
            return [self.push(n) for n in sizes]
        finally:
            self.raw_total, self.k_next = state


class HostDecimator:
    """A stream decimated on the host by the fp64 reference, piece by piece: the carried raw samples are kept in
    fp64 (exact for fp32 and int16 input).  ``push(x)`` returns the fp64 outputs ``[.., m]`` the piece completes."""

    def __init__(self, taps, D: int):
        self.taps = np.asarray(taps, dtype=np.float64)
        self.book = DecimatorBook(len(self.taps), D)
        self.carry: Optional[np.ndarray] = None

    def push(self, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        m, carry_len, skip = self.book.push(x.shape[-1])
        if self.carry is None:
            self.carry = np.zeros(x.shape[:-1] + (0,))
        s = np.concatenate([self.carry[..., :carry_len], x[..., skip:]], -1)
        y = fir_decimate_reference(s, self.taps, self.book.D)
        if y.shape[-1] != m:
            raise AssertionError("the book and the reference disagree")
        self.carry = s[..., m * self.book.D:]
        return y
