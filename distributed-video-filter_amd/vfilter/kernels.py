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


# -- taps for vfilter.sep_filter2d / vfilter.Separable: 1-D, one axis ----------------------------------
# Each builder returns ``(taps, shift)``: a 1-D int16 array and the power of two ONE axis divides
# by.  The shifts of the two axes add and their sum is at most 16.

def binomial_taps(n: int):
    """The binomial row of n taps, ``[1 2 1] / 4``, ``[1 4 6 4 1] / 16``, ...: ``(taps, n - 1)``.  Odd n up to
    9, so that two axes of n - 1 bits each stay within 16 bits.  ``binomial_taps(7)`` on both axes is
    ``gaussian7()`` in 14 taps."""
    n = int(n)
    if n < 1 or n > 9 or n % 2 == 0:
        raise ValueError(f"binomial_taps: n = {n}; n is odd and at most 9")
    row = np.array([1])
    for _ in range(n - 1):
        row = np.convolve(row, [1, 1])
    return row.astype(np.int16), n - 1


def gaussian_taps(ksize: int, sigma: float, bits: int = 8):
    """A sampled Gaussian of ``ksize`` taps (odd, at most 31) and standard deviation ``sigma`` in fixed
    point: ``(taps, bits)``, symmetric taps that sum to exactly ``2**bits``.

    The quantisation is this project's, not cv2's: the samples ``exp(-x*x / (2 sigma^2))`` are scaled to
    sum to ``2**bits`` and floored, and the units still missing go to the taps with the largest
    remainders, a symmetric pair at a time from the centre outwards on equal remainders (an odd unit
    goes to the centre tap).  ``cv2.GaussianBlur``'s own 8-bit taps may differ in the last unit."""
    ksize, bits = int(ksize), int(bits)
    if ksize < 1 or ksize > 31 or ksize % 2 == 0:
        raise ValueError(f"gaussian_taps: ksize = {ksize}; ksize is odd and at most 31")
    if not 1 <= bits <= 14:  # a tap of 2**bits fits int16
        raise ValueError(f"gaussian_taps: bits = {bits} outside 1..14")
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"gaussian_taps: sigma = {sigma!r} is not a positive number")
    r = ksize // 2
    x = np.arange(r + 1, dtype=np.float64)  # the centre and one side: the other side mirrors it
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g *= float(1 << bits) / (g[0] + 2.0 * g[1:].sum())
    q = np.floor(g).astype(np.int64)
    missing = (1 << bits) - int(q[0] + 2 * q[1:].sum())
    rem = g - q
    order = sorted(range(1, r + 1), key=lambda i: (-rem[i], i))  # side taps: a unit costs two
    while missing >= 2 and order:
        for i in order:
            if missing < 2:
                break
            q[i] += 1
            missing -= 2
    q[0] += missing  # an odd unit, or all of them when ksize == 1
    taps = np.concatenate([q[:0:-1], q])
    assert int(taps.sum()) == 1 << bits
    return taps.astype(np.int16), bits
