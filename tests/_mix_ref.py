"""The numpy reference of the colour matrix (include/vfilter.h "colour matrix"), in
int64.  It shares no code with ``vfilter``.

    acc[c] = sum_k M[c][k] * src[y, x, k] + t[c]
    q      = acc                                   when shift == 0
           = f + ((r > h) or (r == h and f odd))   half_even: f = acc >> shift, r = acc - (f << shift), h = 2^(shift-1)
           = (acc + 2^(shift - 1)) >> shift        half_up
    dst    = min(max(q, 0), 255)
"""
import numpy as np


def mat(rows, t=(0, 0, 0)):
    """The 3 x 4 int64 ``[M | t]`` of three rows and three offsets."""
    m = np.zeros((3, 4), np.int64)
    m[:, :3] = np.asarray(rows, np.int64)
    m[:, 3] = np.asarray(t, np.int64)
    return m


def acc(img, m):
    """The exact accumulators, int64 ``... x 3``."""
    m = np.asarray(m, np.int64)
    assert m.shape == (3, 4) and img.dtype == np.uint8 and img.shape[-1] == 3
    x = img.astype(np.int64)
    return np.stack([x[..., 0] * m[c, 0] + x[..., 1] * m[c, 1] + x[..., 2] * m[c, 2] + m[c, 3] for c in range(3)], axis=-1)


def descale(a, shift, rounding):
    a = np.asarray(a, np.int64)
    if shift == 0:
        return a
    h = np.int64(1) << (shift - 1)
    if rounding == "half_up":
        return (a + h) >> shift
    assert rounding == "half_even", rounding
    f = a >> shift  # floor
    r = a - (f << shift)
    return f + ((r > h) | ((r == h) & ((f & 1) == 1)))


def mix(img, m, shift=0, rounding="half_even"):
    """uint8 ``... x 3`` -> uint8 of the same shape."""
    return np.clip(descale(acc(img, m), shift, rounding), 0, 255).astype(np.uint8)


def mix_float(img, m, shift=0, rounding="half_even"):
    """The same in float64 (exact: |acc| < 2^26 and the scale is a power of two): ``np.rint`` rounds
    half to even, ``floor(x + 0.5)`` half up."""
    m = np.asarray(m, np.float64)
    x = img.astype(np.float64)
    v = (x @ m[:, :3].T + m[:, 3]) / float(1 << shift)
    q = np.rint(v) if rounding == "half_even" else np.floor(v + 0.5)
    return np.clip(q, 0, 255).astype(np.uint8)


# -- the matrices of the tests: name -> (3 x 4 int64, shift) ------------------------------------------

IDENTITY = (mat(np.eye(3)), 0)
SWAP_RB = (mat(np.eye(3)[::-1]), 0)
# ties: acc = b + 2 g + 6 r + 2 over 4 is a tie whenever acc % 4 == 2 (acc = 2: floor 0, even; acc = 6: floor 1, odd)
TIES = (mat([[1, 2, 6], [6, 2, 1], [1, -2, 1]], (2, 2, 2)), 2)


def matrix_set():
    """The hand-made matrices (the ``colors`` presets are added by the tests that may import
    ``vfilter``)."""
    return {
        "identity": IDENTITY,
        "swap_rb": SWAP_RB,
        "all_negative_row": (mat([[-3, -200, -7], [40, 50, 60], [-1, -1, -1]], (255 * 16, 0, 100)), 4),
        "sum_65536_shift_16": (mat([[32767, 32767, 2], [-32768, 32767, 1], [21846, 21845, 21845]],
                                   (255 << 16, 255 << 16, -(255 << 16))), 16),
        "shift0_offsets": (mat([[1, 1, 0], [1, -1, 1], [0, 0, 2]], (255, -255, -255)), 0),
        "ties": TIES,
    }


def tie_frame():
    """A 16 x 16 x 3 frame on which ``TIES`` has exact ties with even and with odd floors."""
    b, g = np.meshgrid(np.arange(16, dtype=np.uint8), np.arange(16, dtype=np.uint8))
    return np.stack([b, g, ((b + 2 * g) % 7).astype(np.uint8)], axis=-1)
