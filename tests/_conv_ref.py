"""The numpy reference of the 2-D convolution filter for the conv tests: ``np.pad`` with the
matching mode, then the integer definition (correlation, anchor at the centre, signed 32-bit sum,
round half to even on the shift, saturate).  A transcription of the definition; shares no code
with ``vfilter``."""
import numpy as np

PAD_MODE = {"reflect101": "reflect", "replicate": "edge", "constant": "constant"}


def pad(src, ry, rx, border):
    """``src`` (H x W x C) with ry rows and rx columns of border on each side.  np.pad's "reflect"
    is reflect-101 and reflects repeatedly when the pad is wider than the axis; on an axis of one
    element (where np.pad cannot reflect) every index is 0: the edge value."""
    out = src
    for axis, r in ((0, ry), (1, rx)):
        if r == 0:
            continue
        mode = PAD_MODE[border]
        if mode == "reflect" and out.shape[axis] == 1:
            mode = "edge"
        width = [(0, 0)] * out.ndim
        width[axis] = (r, r)
        out = np.pad(out, width, mode=mode)
    return out


def accumulate(src, weights, border="reflect101"):
    """acc[y, x, c] = sum_j sum_i K[j, i] * src[by(y + j - kh//2), bx(x + i - kw//2), c], int64."""
    k = np.asarray(weights, dtype=np.int64)
    kh, kw = k.shape
    img = np.asarray(src)
    assert img.dtype == np.uint8
    flat = img.ndim == 2
    if flat:
        img = img[:, :, None]
    h, w, _ = img.shape
    p = pad(img.astype(np.int64), kh // 2, kw // 2, border)
    acc = np.zeros(img.shape, dtype=np.int64)
    for j in range(kh):
        for i in range(kw):
            acc += k[j, i] * p[j:j + h, i:i + w]
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc[:, :, 0] if flat else acc


def round_shift(acc, shift):
    """round_half_even(acc / 2^shift) by the definition's integer steps."""
    if shift == 0:
        return acc
    f = acc >> shift  # arithmetic: floor
    r = acc & ((1 << shift) - 1)
    h = 1 << (shift - 1)
    return f + ((r > h) | ((r == h) & ((f & 1) == 1)))


def filter2d(src, weights, shift=0, border="reflect101"):
    q = round_shift(accumulate(src, weights, border), shift)
    return np.clip(q, 0, 255).astype(np.uint8)


def stats(src, weights, shift=0, border="reflect101"):
    """(ties, negative accumulators, saturated outputs) of the reference on this input."""
    acc = accumulate(src, weights, border)
    q = round_shift(acc, shift)
    ties = int(((acc & ((1 << shift) - 1)) == (1 << (shift - 1))).sum()) if shift else 0
    return ties, int((acc < 0).sum()), int(((q < 0) | (q > 255)).sum())


def filter2d_float32(src, weights, shift=0, border="reflect101"):
    """What cv2.filter2D(src, -1, K / 2^shift) does: float32 kernel, float32 accumulation, round to
    nearest even (cvRound), saturate."""
    k = (np.asarray(weights, dtype=np.float32) / np.float32(2 ** shift)).astype(np.float32)
    kh, kw = k.shape
    img = np.asarray(src)
    flat = img.ndim == 2
    if flat:
        img = img[:, :, None]
    h, w, _ = img.shape
    p = pad(img, kh // 2, kw // 2, border).astype(np.float32)
    acc = np.zeros(img.shape, dtype=np.float32)
    for j in range(kh):
        for i in range(kw):
            acc = (acc + k[j, i] * p[j:j + h, i:i + w]).astype(np.float32)
    out = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def kernel_set():
    """The kernels the GPU tests use, as name -> (int weights, shift)."""
    r7 = np.random.default_rng(77).integers(-300, 301, (7, 7))
    r35 = np.random.default_rng(35).integers(-9, 10, (5, 3))  # 3 wide x 5 high
    g3 = np.outer([1, 2, 1], [1, 2, 1])
    b5 = np.array([1, 4, 6, 4, 1])
    return {
        "gaussian3": (g3, 4),
        "gaussian5": (np.outer(b5, b5), 8),
        "sharpen": (np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]]), 0),
        "sobel_x": (np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]), 1),
        "random7": (r7, 9),
        "random3x5": (r35, 3),
    }



OBLONG_SIDES = [(1, 3), (1, 7), (7, 1), (5, 1), (7, 3), (3, 7), (5, 3), (1, 1)]  # kh x kw


def oblong_set():
    """Kernels that are not square, most of them wider than tall, as name "khxkw" -> (int weights,
    shift): random signed weights, so a flip, a transpose or a kernel put off-centre into the
    square the GPU kernel is compiled for cannot pass.  7x3 sums |K| above 128 (the wide form)."""
    out = {}
    for kh, kw in OBLONG_SIDES:
        rng = np.random.default_rng([16, kh, kw])
        m = 60 if (kh, kw) == (7, 3) else 9
        k = rng.integers(-m, m + 1, (kh, kw))
        if kh * kw == 1:
            k[0, 0] = 3  # 1x1: a gain of 3 / 8
        out["%dx%d" % (kh, kw)] = (k, 8 if m == 60 else 1 + (kh + kw) % 3)
    assert np.abs(out["7x3"][0]).sum() > 128 >= np.abs(out["1x7"][0]).sum()
    return out
