"""Ready-made kernels for ``vfilter.filter2d`` (the ``cv2.filter2D`` drop-in), analogous to
``vfilter.tables`` for ``vfilter.lut``.

Every builder returns ``(weights, shift)``: an int16 ``kh x kw`` array and the power of two the
sum is divided by, i.e. the kernel ``weights / 2**shift`` evaluated exactly (round half to even,
saturate).  All of them are accepted as they are by ``filter2d``, ``TurboJPEG.filter2d*`` and
``ConvWorker``.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def _k(rows, shift=0):
    return np.array(rows, dtype=np.int16), int(shift)


def identity():
    """The 1 x 1 kernel [1]: the frame itself."""
    return _k([[1]])


def box(n: int):
    """The n x n mean.  Only for the n whose divisor n * n is a power of two; among the odd sides
    up to 7 that is n = 1 alone (a 3 x 3 mean is 1/9: not dyadic), so every other n raises."""
    n = int(n)
    if n < 1 or n > 7 or n % 2 == 0:
        raise ValueError(f"box: n = {n}; sides are odd and at most 7")
    area = n * n
    if area & (area - 1):
        raise ValueError(f"box: 1/{area} is not dyadic; use gaussian{n}() or an integer kernel with a shift")
    return _k(np.ones((n, n)), area.bit_length() - 1)


def _binomial(n: int):
    row = np.array([1])
    for _ in range(n - 1):
        row = np.convolve(row, [1, 1])
    return _k(np.outer(row, row), 2 * (n - 1))


def gaussian3():
    """[1 2 1] x [1 2 1] / 16."""
    return _binomial(3)


def gaussian5():
    """[1 4 6 4 1] x [1 4 6 4 1] / 256."""
    return _binomial(5)


def gaussian7():
    """[1 6 15 20 15 6 1] x [1 6 15 20 15 6 1] / 4096."""
    return _binomial(7)


def sharpen():
    """The 4-neighbour sharpening kernel: 5 at the centre, -1 above, below, left and right."""
    return _k([[0, -1, 0], [-1, 5, -1], [0, -1, 0]])


def laplacian():
    """The 4-neighbour Laplacian (cv2.Laplacian with ksize = 1)."""
    return _k([[0, 1, 0], [1, -4, 1], [0, 1, 0]])


def sobel_x():
    """The 3 x 3 Sobel derivative along x (negative results saturate to 0, as in uint8 cv2.filter2D)."""
    return _k([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])


def sobel_y():
    """The 3 x 3 Sobel derivative along y."""
    return _k([[-1, -2, -1], [0, 0, 0], [1, 2, 1]])


def emboss():
    return _k([[-2, -1, 0], [-1, 1, 1], [0, 1, 2]])


def unsharp(amount=1):
    """Unsharp mask with the 3 x 3 Gaussian: ``(1 + amount) * identity - amount * gaussian3``.
    ``amount`` must be dyadic (an integer, 0.5, 0.25, 1.5, ...) so that the kernel is exact."""
    a = Fraction(amount).limit_denominator(1 << 20) if not isinstance(amount, Fraction) else amount
    if float(a) != float(amount) or a.denominator & (a.denominator - 1) or a < 0:
        raise ValueError(f"unsharp: amount = {amount!r} is not a non-negative dyadic number")
    s = a.denominator.bit_length() - 1  # amount = num / 2^s
    g, gs = gaussian3()                 # / 16
    ident = np.zeros((3, 3), dtype=np.int64)
    ident[1, 1] = 1
    # ((2^s + num) * 16 * identity - num * g) / 2^(s + 4)
    w = (a.denominator + a.numerator) * 16 * ident - a.numerator * g.astype(np.int64)
    shift = s + gs
    while shift > 0 and not (w & 1).any():  # smallest shift
        w >>= 1
        shift -= 1
    if shift > 16 or np.abs(w).sum() > 65536:
        raise ValueError(f"unsharp: amount = {amount!r} needs more precision than a kernel holds")
    return w.astype(np.int16), shift
