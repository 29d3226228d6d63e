"""Builders of 256-entry filter tables for ``vfilter.lut`` (``cv2.LUT`` on the MI355X).

Every per-pixel filter of 8-bit frames is such a table: what the reference's plugin slot holds
as ``cv2.bitwise_not(frame)`` (inverter.py:41) becomes ``vfilter.lut(frame, tables.gamma(2.2))``
and so on.  Pure numpy, no GPU; each builder returns a ``(256,)`` uint8 array, and ``stack``
puts three of them together as the ``(256, 3)`` per-channel table of a BGR frame.
"""
from __future__ import annotations

import numpy as np

_V = np.arange(256, dtype=np.float64)


def _u8(x) -> np.ndarray:
    """saturate_cast<uchar> of doubles: round half to even (cvRound), then clamp."""
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def identity() -> np.ndarray:
    return np.arange(256, dtype=np.uint8)


def invert() -> np.ndarray:
    """``cv2.bitwise_not`` as a table."""
    return (255 - np.arange(256)).astype(np.uint8)


def gamma(g: float) -> np.ndarray:
    """``255 * (v / 255) ** (1 / g)``: g > 1 brightens the mid-tones (display gamma correction)."""
    if not g > 0:
        raise ValueError("gamma: g must be positive")
    return _u8(255.0 * (_V / 255.0) ** (1.0 / float(g)))


def levels(alpha: float, beta: float = 0.0) -> np.ndarray:
    """Contrast ``alpha`` and brightness ``beta`` with ``cv2.convertScaleAbs`` semantics:
    ``saturate(round_half_even(|alpha * v + beta|))``."""
    return _u8(np.abs(float(alpha) * _V + float(beta)))


def threshold(t: int) -> np.ndarray:
    """``cv2.threshold(..., t, 255, THRESH_BINARY)``: 255 where v > t, else 0."""
    return np.where(np.arange(256) > int(t), 255, 0).astype(np.uint8)


def posterize(bits: int) -> np.ndarray:
    """Keep the top ``bits`` bits of every value (1..8; 8 is the identity)."""
    bits = int(bits)
    if not 1 <= bits <= 8:
        raise ValueError("posterize: bits must be 1..8")
    mask = (0xFF << (8 - bits)) & 0xFF
    return (np.arange(256) & mask).astype(np.uint8)


def stack(b, g, r) -> np.ndarray:
    """The ``(256, 3)`` table of a BGR frame from one ``(256,)`` table per channel."""
    cols = [np.asarray(t) for t in (b, g, r)]
    for t in cols:
        if t.dtype != np.uint8 or t.shape != (256,):
            raise ValueError("stack: each table must be (256,) uint8")
    return np.stack(cols, axis=1)
