"""The resize (``cv2.resize`` on 8-bit frames of 1 or 3 channels) in numpy, written from the rule's definition
(DESIGN.md 26.1): nearest, linear in cv2's 11-bit fixed point, and area for integer shrink factors.  Every float
and double operation is a numpy scalar or array operation of that type, so each rounds on its own; nothing here
shares code with ``csrc/vf_resize_plan.h``.  The GPU tests compare the library against this, byte for byte.
"""
import numpy as np

NEAREST, LINEAR, AREA = 0, 1, 3
MAX_SIDE = 32767
MAX_AREA_FACTOR = 16
DBL_EPSILON = float(np.finfo(np.float64).eps)


def _rint_int(v):
    """rint (half to even) of a float64, saturated to int32."""
    r = np.rint(np.float64(v))
    return int(min(max(r, -2147483648.0), 2147483647.0))


def out_size(w, h, dsize=None, fx=0.0, fy=0.0):
    """(dw, dh) of a frame of w x h."""
    if dsize:
        return int(dsize[0]), int(dsize[1])
    return _rint_int(np.float64(w) * np.float64(fx)), _rint_int(np.float64(h) * np.float64(fy))


def scales(w, h, dsize=None, fx=0.0, fy=0.0):
    """(scale_x, scale_y) as float64: 1 / (dw / W) with a dsize, 1 / fx without."""
    if dsize:
        inv_x, inv_y = np.float64(dsize[0]) / np.float64(w), np.float64(dsize[1]) / np.float64(h)
        return np.float64(1.0) / inv_x, np.float64(1.0) / inv_y
    return np.float64(1.0) / np.float64(fx), np.float64(1.0) / np.float64(fy)


def integer_scale(scale):
    """cv2's test, literally: (whether |scale - rint(scale)| < DBL_EPSILON, rint(scale))."""
    i = _rint_int(scale)
    return bool(abs(np.float64(scale) - np.float64(i)) < DBL_EPSILON), i


def resolve(w, h, dsize=None, fx=0.0, fy=0.0, interp=LINEAR):
    """(mode after cv2's substitution, scale_x, scale_y, iscale_x, iscale_y); ValueError for an area that is not built."""
    sx, sy = scales(w, h, dsize, fx, fy)
    (okx, ix), (oky, iy) = integer_scale(sx), integer_scale(sy)
    fast = okx and oky
    mode = interp
    if interp == LINEAR and fast and ix == 2 and iy == 2:
        mode = AREA
    if mode == AREA and not (fast and sx >= 1 and sy >= 1 and ix <= MAX_AREA_FACTOR and iy <= MAX_AREA_FACTOR):
        raise ValueError("area is built for integer shrink factors of 1 to 16 only")
    return mode, sx, sy, ix, iy


def nearest_index(scale, n_dst, n_src):
    d = np.arange(n_dst, dtype=np.float64)
    return np.minimum(np.floor(d * np.float64(scale)), n_src - 1).astype(np.int64)


def axis_coef(scale, n_dst, n_src, edge_reset):
    """(s, w0, w1) of every destination index: columns reset the fraction at both edges, rows do not."""
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + np.float64(0.5)) * np.float64(scale) - np.float64(0.5)).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = (f - fl).astype(np.float32)
    if edge_reset:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= n_src - 1
        f[hi], s[hi] = 0, n_src - 1
    one, k = np.float32(1.0), np.float32(2048.0)
    w0 = np.clip(np.rint(((one - f).astype(np.float32) * k).astype(np.float32)), -32768, 32767).astype(np.int64)
    w1 = np.clip(np.rint((f * k).astype(np.float32)), -32768, 32767).astype(np.int64)
    return s, w0, w1


def _planes(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return img.reshape(img.shape[0], img.shape[1], -1)


def _linear(src, dw, dh, sx, sy):
    h, w, _ = src.shape
    cs, a0, a1 = axis_coef(sx, dw, w, True)
    rs, b0, b1 = axis_coef(sy, dh, h, False)
    s = src.astype(np.int64)
    hrow = s[:, cs, :] * a0[None, :, None] + s[:, np.minimum(cs + 1, w - 1), :] * a1[None, :, None]  # int32 range
    h0 = hrow[np.clip(rs, 0, h - 1)] >> 4
    h1 = hrow[np.clip(rs + 1, 0, h - 1)] >> 4
    out = (((b0[:, None, None] * h0) >> 16) + ((b1[:, None, None] * h1) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def _sat_u8_rint(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _area(src, dw, dh, ix, iy):
    h, w, c = src.shape
    out = np.zeros((dh, dw, c), np.uint8)
    whole_cols = w // ix
    inv = np.float32(1.0) / np.float32(ix * iy)
    for dy in range(dh):
        y0 = dy * iy
        row_whole = y0 + iy <= h
        for dx in range(dw):
            x0 = dx * ix
            block = src[y0:min(y0 + iy, h), x0:min(x0 + ix, w), :].astype(np.int64)
            total, count = block.sum(axis=(0, 1)), block.shape[0] * block.shape[1]
            if row_whole and dx < whole_cols:
                if ix == 2 and iy == 2:
                    out[dy, dx] = (total + 2) >> 2
                else:
                    out[dy, dx] = _sat_u8_rint((total.astype(np.float32) * inv).astype(np.float32))
            elif count:  # cv2's slow tail: the pixels inside the frame, their float sum over their count
                out[dy, dx] = _sat_u8_rint((total.astype(np.float32) / np.float32(count)).astype(np.float32))
    return out


def resize(img, dsize=None, fx=0.0, fy=0.0, interp=LINEAR):
    """The resized frame; ``dsize`` is (width, height) as cv2's."""
    src = _planes(img)
    h, w, _ = src.shape
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError("a side is 1 to 32767")
    dw, dh = out_size(w, h, dsize, fx, fy)
    if dw < 1 or dh < 1:
        raise ValueError("a side of 0")
    if dw > MAX_SIDE or dh > MAX_SIDE:
        raise ValueError("a side is at most 32767")
    mode, sx, sy, ix, iy = resolve(w, h, dsize, fx, fy, interp)
    if mode == NEAREST:
        out = src[nearest_index(sy, dh, h)][:, nearest_index(sx, dw, w)]
    elif mode == LINEAR:
        out = _linear(src, dw, dh, sx, sy)
    else:
        out = _area(src, dw, dh, ix, iy)
    return np.ascontiguousarray(out if np.asarray(img).ndim == 3 else out[:, :, 0])
