"""The numpy reference of the rank filters (erode, dilate, median) for the rank tests: a
transcription of the definition in DESIGN.md 18; shares no code with ``vfilter``.

erode / dilate: the frame padded with ``np.pad`` in the matching mode -- for "constant" with the
operation's neutral value, 255 for the minimum and 0 for the maximum, which is what "a tap outside
the frame is left out of the set" comes to, the empty set included -- then ``np.minimum`` /
``np.maximum`` over the member offsets.  median: edge padding, the ``ksize**2`` shifted views
stacked, sorted along the stack, the middle taken.  The handling of a one-element axis under
reflect is ``tests/_conv_ref.py``'s ``pad``."""
import numpy as np

from _conv_ref import pad as _pad

BORDERS = ("reflect101", "replicate", "constant")


def _morph(src, element, border, is_max):
    e = np.asarray(element) != 0
    kh, kw = e.shape
    assert kh % 2 == 1 and kw % 2 == 1 and e.any()
    img = np.asarray(src)
    assert img.dtype == np.uint8
    flat = img.ndim == 2
    if flat:
        img = img[:, :, None]
    h, w, _ = img.shape
    ry, rx = kh // 2, kw // 2
    if border == "constant":
        p = np.pad(img, ((ry, ry), (rx, rx), (0, 0)), mode="constant", constant_values=0 if is_max else 255)
    else:
        p = _pad(img, ry, rx, border)
    out = np.full(img.shape, 0 if is_max else 255, dtype=np.uint8)
    for j in range(kh):
        for i in range(kw):
            if e[j, i]:
                out = (np.maximum if is_max else np.minimum)(out, p[j:j + h, i:i + w])
    return out[:, :, 0] if flat else out


def erode(src, element, border="constant"):
    return _morph(src, element, border, False)


def dilate(src, element, border="constant"):
    return _morph(src, element, border, True)


def median(src, ksize):
    img = np.asarray(src)
    assert img.dtype == np.uint8 and ksize % 2 == 1
    flat = img.ndim == 2
    if flat:
        img = img[:, :, None]
    h, w, _ = img.shape
    r = ksize // 2
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
    stack = np.stack([p[j:j + h, i:i + w] for j in range(ksize) for i in range(ksize)])
    out = np.sort(stack, axis=0)[ksize * ksize // 2]
    return out[:, :, 0] if flat else out


def apply(src, op, arg, border="constant"):
    """op "erode" / "dilate" with an element, or "median" with a ksize."""
    if op == "median":
        return median(src, arg)
    return (erode if op == "erode" else dilate)(src, arg, border)


def rect(w, h=None):
    return np.ones((w if h is None else h, w), np.uint8)


def cross(w, h=None):
    h = w if h is None else h
    e = np.zeros((h, w), np.uint8)
    e[h // 2, :] = 1
    e[:, w // 2] = 1
    return e


def element_set():
    """The elements the GPU tests use, by name.  random7 (its centre is not a member) and corner5
    (only the top-left corner) make a flip, a transpose or a wrong anchor fail, and leave the set
    empty near an edge under the constant border."""
    r7 = (np.random.default_rng(707).integers(0, 2, (7, 7)) != 0).astype(np.uint8)
    r7[3, 3] = 0
    assert r7.any() and not np.array_equal(r7, r7.T) and not np.array_equal(r7, r7[::-1, ::-1])
    c5 = np.zeros((5, 5), np.uint8)
    c5[0, 0] = 1
    return {"rect3": rect(3), "rect5": rect(5), "rect7": rect(7), "cross3": cross(3), "cross5": cross(5),
            "rect3x5": rect(3, 5), "random7": r7, "corner5": c5}


OBLONG_SIDES = [(1, 3), (1, 7), (7, 1), (5, 1), (7, 3), (3, 7), (5, 3), (1, 1)]  # kh x kw


def oblong_set():
    """Elements that are not square, most of them wider than tall, as name "khxkw" -> element:
    random members (1x7 and 7x1 without their centre, and not symmetric), so a flip, a transpose or
    an element put off-centre into the square the GPU kernel is compiled for cannot pass."""
    out = {}
    for kh, kw in OBLONG_SIDES:
        e = (np.random.default_rng([18, kh, kw]).integers(0, 2, (kh, kw)) != 0).astype(np.uint8)
        if (kh, kw) in ((1, 7), (7, 1), (3, 7)):
            e[kh // 2, kw // 2] = 0
            e.flat[0], e.flat[-1] = 1, 0
        if kh * kw > 1 and e.sum() < 2:  # more than the identity
            e.flat[0] = 1
        if not e.any():
            e[kh // 2, kw // 2] = 1
        out["%dx%d" % (kh, kw)] = e
    for name in ("1x7", "7x1", "3x7"):
        assert not out[name][out[name].shape[0] // 2, out[name].shape[1] // 2]
        assert not np.array_equal(out[name], out[name][::-1, ::-1])
    return out
