"""Builders of the usual colour matrices for ``vfilter.transform`` / ``vfilter.Mix``.

Every builder returns what ``Mix`` and ``transform`` take: an ``(ints, shift)`` pair, ``ints`` an int64
3 x 4 array ``[M | t]`` that means ``[M | t] / 2**shift``, or -- where a rounding belongs to the
preset -- a ``Mix`` value that carries it.  Frames are BGR, as the reference's are: channel 0 is
blue, row c of the matrix makes output channel c.  Each docstring gives the integers.
"""
from __future__ import annotations

import numpy as np

from .filters import Mix

# Rec. 601 luma 0.114 B + 0.587 G + 0.299 R in 15 bits, the integers OpenCV 4.x's 8-bit
# cvtColor(BGR2GRAY) uses (DESIGN.md 20.1 argues this from its source; it is not measured here).
_GRAY15 = (3735, 19235, 9798)
# the same luma rounded to /256 so that the row sums to 256: 29 + 150 + 77
_LUMA8 = (29, 150, 77)


def _pair(rows, offsets=(0, 0, 0), shift: int = 0) -> tuple:
    m = np.zeros((3, 4), np.int64)
    m[:, :3] = rows
    m[:, 3] = offsets
    return m, shift


def _dyadic(name: str, v, most: int = 8) -> tuple:
    """``v`` as ``(integer, shift)`` with the smallest shift in 0..most; raises when there is none."""
    v = float(v)
    if not np.isfinite(v):
        raise ValueError(f"{name}: {v!r} is not finite")
    for s in range(most + 1):
        if v * (1 << s) == np.rint(v * (1 << s)):
            return int(np.rint(v * (1 << s))), s
    raise ValueError(f"{name}: {v!r} is not dyadic (no s in 0..{most} makes it * 2**s integral)")


def identity() -> tuple:
    """The identity: rows (1, 0, 0), (0, 1, 0), (0, 0, 1), offset 0, shift 0."""
    return _pair(np.eye(3, dtype=np.int64))


def swap_rb() -> tuple:
    """BGR <-> RGB: rows (0, 0, 1), (0, 1, 0), (1, 0, 0), offset 0, shift 0."""
    return _pair(np.eye(3, dtype=np.int64)[::-1])


def gray_weights(b: int, g: int, r: int, shift: int) -> tuple:
    """Grayscale kept in 3 channels with the caller's luma: the row ``(b, g, r)`` in all three rows,
    offset 0, over ``2**shift``.  ``gray_weights(1868, 9617, 4899, 14)`` is the 14-bit luma of OpenCV
    2.4 -- 3.x's ``CV_DESCALE`` path."""
    for v in (b, g, r, shift):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"gray_weights: integers, not {v!r}")
    return _pair([[b, g, r]] * 3, shift=int(shift))


def gray() -> Mix:
    """``cv2.cvtColor(src, cv2.COLOR_BGR2GRAY)`` copied into 3 channels: the row (3735, 19235, 9798)
    in all three rows, shift 15, rounding half_up -- ``(3735 B + 19235 G + 9798 R + 16384) >> 15``, the
    fixed-point form of OpenCV 4.x (argued in DESIGN.md 20.1, not measured)."""
    return Mix(gray_weights(*_GRAY15, 15), "half_up")


def sepia() -> tuple:
    """The usual sepia matrix (R' = .393 R + .769 G + .189 B, G' = .349 R + .686 G + .168 B,
    B' = .272 R + .534 G + .131 B) rounded to /256, as such -- it is this project's rounding, not a
    cv2 preset.  In BGR order, rows for B', G', R': (34, 137, 70), (43, 176, 89), (48, 197, 101),
    offset 0, shift 8."""
    return _pair([[34, 137, 70], [43, 176, 89], [48, 197, 101]], shift=8)


def saturation(s) -> tuple:
    """``s * I + (1 - s) * L`` for a dyadic ``s`` in 0..4 (0: gray, 1: identity, 2: doubled), ``L`` the
    /256 luma row (29, 150, 77) in every row.  With ``s = n / 2**k`` (k <= 8) the integers are
    ``256 n I + (2**k - n) L`` over shift ``8 + k``; e.g. ``saturation(0.5)`` is ``256 I + L`` over 512:
    rows (285, 150, 77), (29, 406, 77), (29, 150, 333), shift 9.  ``Mix`` refuses a result whose
    weights leave 16 bits (a large ``s`` with many fractional bits)."""
    n, k = _dyadic("saturation", s)
    if not 0 <= n <= 4 << k:
        raise ValueError(f"saturation: s = {s!r} outside 0..4")
    rows = 256 * n * np.eye(3, dtype=np.int64) + ((1 << k) - n) * np.array([_LUMA8] * 3, np.int64)
    return _pair(rows, shift=8 + k)


def gain(b, g, r) -> tuple:
    """White balance: channel c times its dyadic gain in 0..127 (at most 8 fractional bits): the
    diagonal ``(b, g, r) * 2**shift`` with the smallest common shift, offset 0; e.g. ``gain(1, 1.5,
    0.75)`` is diag(4, 6, 3), shift 2."""
    parts = [_dyadic("gain", v) for v in (b, g, r)]
    shift = max(s for _, s in parts)
    diag = [n << (shift - s) for n, s in parts]
    if any(d < 0 or d > 32767 for d in diag):
        raise ValueError(f"gain: gains ({b!r}, {g!r}, {r!r}) outside 0..127 at shift {shift}")
    return _pair(np.diag(np.array(diag, np.int64)), shift=shift)


def offset(b: int, g: int, r: int) -> tuple:
    """Add the integers ``(b, g, r)``, each in -255..255, to the channels and clamp: the identity with
    offset (b, g, r), shift 0."""
    for v in (b, g, r):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -255 <= v <= 255:
            raise ValueError(f"offset: integers in -255..255, not {v!r}")
    return _pair(np.eye(3, dtype=np.int64), (b, g, r))
