"""The numpy reference of the affine warp, written from the rule's text (the classic fixed-point
path of OpenCV 3.x .. 4.10 ``imgwarp.cpp`` for 8-bit frames, ``AB_BITS = 10``, ``INTER_BITS = 5``, 15-bit weights),
not from ``csrc/vf_warp_plan.h``.  ``m`` is the map from destination to source.  Every double operation below is a
numpy float64 operation of its own, so none is fused; ``np.rint`` rounds half to even."""
import numpy as np

LINEAR, NEAREST = 0, 1
REFLECT101, REPLICATE, CONSTANT = 0, 1, 2  # VF_BORDER_*
AFFINE, FLIP_H, FLIP_V, FLIP_BOTH = 0, 1, 2, 3


def resolve(mode, m, w, h):
    if mode == AFFINE:
        return [float(v) for v in np.asarray(m, np.float64).reshape(6)]
    if mode == FLIP_H:
        return [-1.0, 0.0, float(w - 1), 0.0, 1.0, 0.0]
    if mode == FLIP_V:
        return [1.0, 0.0, 0.0, 0.0, -1.0, float(h - 1)]
    return [-1.0, 0.0, float(w - 1), 0.0, -1.0, float(h - 1)]


def _to_int(v):
    """rint, then the saturating conversion to int32 (kept in int64 so that the sums below cannot wrap)."""
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def coords(m, w, h, interp):
    """(sx, sy, fx, fy), each H x W int64: the first tap and the fractions in 1 / 32 (0 for nearest)."""
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in m)
    x = np.arange(w, dtype=np.float64)
    y = np.arange(h, dtype=np.float64)
    rd = 512 if interp == NEAREST else 16
    adelta = _to_int((m0 * x) * 1024.0)[None, :]
    bdelta = _to_int((m3 * x) * 1024.0)[None, :]
    x0 = (_to_int((m1 * y + m2) * 1024.0) + rd)[:, None]
    y0 = (_to_int((m4 * y + m5) * 1024.0) + rd)[:, None]
    if interp == NEAREST:
        sx = np.clip((x0 + adelta) >> 10, -32768, 32767)
        sy = np.clip((y0 + bdelta) >> 10, -32768, 32767)
        return sx, sy, np.zeros_like(sx), np.zeros_like(sy)
    big_x, big_y = (x0 + adelta) >> 5, (y0 + bdelta) >> 5
    return np.clip(big_x >> 5, -32768, 32767), np.clip(big_y >> 5, -32768, 32767), big_x & 31, big_y & 31


def border_index(p, n, border):
    """The index each position of ``p`` reads on an axis of ``n``, -1 where the constant border applies."""
    p = np.asarray(p, np.int64)
    inside = (p >= 0) & (p < n)
    if border == CONSTANT:
        return np.where(inside, p, -1)
    if border == REPLICATE:
        return np.clip(p, 0, n - 1)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def _taps(img3, ty, tx, border, value):
    h, w, c = img3.shape
    iy, ix = border_index(ty, h, border), border_index(tx, w, border)
    out = img3[np.maximum(iy, 0), np.maximum(ix, 0)].astype(np.int64)  # H x W x C
    outside = (iy < 0) | (ix < 0)
    if outside.any():
        out[outside] = np.asarray(value[:c], np.int64)
    return out


def warp(img, m=None, mode=AFFINE, interp=LINEAR, border=CONSTANT, value=(0, 0, 0)):
    """The warp of a uint8 ``H x W`` or ``H x W x 3`` frame."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.size == 0:
        return img.copy()
    img3 = img[:, :, None] if img.ndim == 2 else img
    h, w = img3.shape[:2]
    value = tuple(int(v) for v in (value if np.ndim(value) else (value,) * 3))
    sx, sy, fx, fy = coords(resolve(mode, m, w, h), w, h, interp)
    if interp == NEAREST:
        out = _taps(img3, sy, sx, border, value)
    else:
        fx, fy = fx[:, :, None], fy[:, :, None]
        acc = 32 * (32 - fx) * (32 - fy) * _taps(img3, sy, sx, border, value)
        acc += 32 * fx * (32 - fy) * _taps(img3, sy, sx + 1, border, value)
        acc += 32 * (32 - fx) * fy * _taps(img3, sy + 1, sx, border, value)
        acc += 32 * fx * fy * _taps(img3, sy + 1, sx + 1, border, value)
        out = (acc + 16384) >> 15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape(img.shape)


def invert_affine(mat):
    """cv2.warpAffine's own inversion of a forward 2 x 3 map, in its order of operations, on Python floats."""
    m0, m1, m2, m3, m4, m5 = (float(v) for v in np.asarray(mat, np.float64).reshape(6))
    d = m0 * m4 - m1 * m3
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m4 * d, m0 * d
    m0, m1, m3, m4 = a11, m1 * -d, m3 * -d, a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return [m0, m1, b1, m3, m4, b2]


def rotation(center, angle, scale):
    """cv2.getRotationMatrix2D."""
    rad = angle * np.pi / 180.0
    a, b = scale * np.cos(rad), scale * np.sin(rad)
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)
