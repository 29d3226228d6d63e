"""The numpy references of the tests against an independent implementation: ``scipy.ndimage``.

``tests/_conv_ref.py``, ``tests/_rank_ref.py`` and ``tests/_chain_ref.py`` are transcriptions of
DESIGN.md 16-19 and share their author with the kernels they judge.  ``scipy.ndimage`` implements
the same four operations on its own:

    _conv_ref.accumulate   ndimage.correlate on int64 (a correlation, the origin at the centre)
    _rank_ref.erode        ndimage.minimum_filter with the element as footprint
    _rank_ref.dilate       ndimage.maximum_filter
    _rank_ref.median       ndimage.median_filter, size k x k

with the modes ``mirror`` for reflect101 (scipy's ``reflect`` repeats the edge pixel), ``nearest``
for replicate and ``constant`` for constant -- ``cval`` 0 for the convolution, 255 for the minimum
and 0 for the maximum, which is "a tap outside the frame is left out of the set".  Every comparison
is exact, over the three borders, square and oblong sides 1 to 7, and frames with axes of length 1
and axes shorter than the radius.  cv2 itself is not measured here.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _conv_ref
import _rank_ref

ndimage = pytest.importorskip("scipy.ndimage")

MODE = {"reflect101": "mirror", "replicate": "nearest", "constant": "constant"}
SIDES = (1, 3, 5, 7)
SHAPES_KH_KW = [(kh, kw) for kh in SIDES for kw in SIDES]  # square and oblong, 1 x 1 included
# (h, w, c): axes of length 1, axes shorter than the radius 3, odd sizes
FRAMES = [(1, 1, 1), (1, 9, 1), (9, 1, 3), (2, 3, 3), (3, 2, 1), (5, 4, 3), (13, 17, 1), (13, 17, 3)]


def _per_channel(img, fn):
    if img.ndim == 2:
        return fn(img)
    return np.stack([fn(img[:, :, c]) for c in range(img.shape[2])], axis=2)


@pytest.mark.parametrize("border", CR.BORDERS)
def test_accumulate_is_ndimage_correlate(border):
    rng = np.random.default_rng(161)
    n = 0
    for kh, kw in SHAPES_KH_KW:
        k = rng.integers(-300, 301, (kh, kw))
        for h, w, c in FRAMES:
            img = CR.noise(h, w, c, seed=kh * 8 + kw)
            want = _per_channel(img, lambda p: ndimage.correlate(p.astype(np.int64), k.astype(np.int64), mode=MODE[border], cval=0))
            got = _conv_ref.accumulate(img, k, border)
            assert got.dtype == np.int64 and np.array_equal(got, want), (border, kh, kw, img.shape)
            n += 1
    assert n == 16 * len(FRAMES)


@pytest.mark.parametrize("border", CR.BORDERS)
def test_erode_and_dilate_are_the_minimum_and_maximum_filters(border):
    rng = np.random.default_rng(162)
    for kh, kw in SHAPES_KH_KW:
        e = (rng.integers(0, 2, (kh, kw)) != 0).astype(np.uint8)
        if kh * kw > 1:
            e[kh // 2, kw // 2] = (kh + kw) // 2 % 2  # the centre is not always a member
        if not e.any():
            e[0, 0] = 1
        for h, w, c in FRAMES:
            img = CR.noise(h, w, c, seed=kh * 8 + kw)
            lo = _per_channel(img, lambda p: ndimage.minimum_filter(p, footprint=e != 0, mode=MODE[border], cval=255))
            hi = _per_channel(img, lambda p: ndimage.maximum_filter(p, footprint=e != 0, mode=MODE[border], cval=0))
            assert np.array_equal(_rank_ref.erode(img, e, border), lo), ("erode", border, e.tolist(), img.shape)
            assert np.array_equal(_rank_ref.dilate(img, e, border), hi), ("dilate", border, e.tolist(), img.shape)


def test_median_is_the_median_filter():
    for ksize in (3, 5):
        for h, w, c in FRAMES:
            img = CR.noise(h, w, c, seed=ksize)
            want = _per_channel(img, lambda p: ndimage.median_filter(p, size=(ksize, ksize), mode="nearest"))
            assert np.array_equal(_rank_ref.median(img, ksize), want), (ksize, img.shape)
    # ties and both extremes in every window
    ext = np.random.default_rng(163).choice(np.array([0, 1, 254, 255], np.uint8), (13, 17))
    assert np.array_equal(_rank_ref.median(ext, 5), ndimage.median_filter(ext, size=(5, 5), mode="nearest"))


def _round_half_even_shift(acc, shift):
    """round_half_even(acc / 2^shift) in floating point: exact, |acc| < 2^31 and 2^shift <= 2^16."""
    return np.rint(acc.astype(np.float64) / float(1 << shift)).astype(np.int64)


def test_the_rounding_is_round_half_to_even():
    acc = np.arange(-5000, 5000, dtype=np.int64)
    for shift in range(0, 9):
        assert np.array_equal(_conv_ref.round_shift(acc, shift), _round_half_even_shift(acc, shift)), shift


@pytest.mark.parametrize("border", CR.BORDERS)
def test_a_whole_chain_from_the_scipy_calls(border):
    """``dog``: absdiff(gaussian3 x, gaussian5 x) through the gamma table, and ``edges``: the median,
    the morphological gradient and a threshold -- put together from ndimage calls and plain numpy."""
    img = CR.noise(13, 17, 3)
    ps = CR.program_set(border, 3)
    g3, g5 = _conv_ref.kernel_set()["gaussian3"], _conv_ref.kernel_set()["gaussian5"]

    def blur(p, k, shift):
        acc = ndimage.correlate(p.astype(np.int64), np.asarray(k, np.int64), mode=MODE[border], cval=0)
        return np.clip(_round_half_even_shift(acc, shift), 0, 255)

    def dog(p):
        return CR.gamma_table(0.5)[np.abs(blur(p, *g3) - blur(p, *g5))]

    assert np.array_equal(CR.run(img, ps["dog"]), _per_channel(img, dog))

    def edges(p):
        m = ndimage.median_filter(p, size=(3, 3), mode="nearest")
        hi = ndimage.maximum_filter(m, size=(3, 3), mode=MODE[border], cval=0).astype(np.int64)
        lo = ndimage.minimum_filter(m, size=(3, 3), mode=MODE[border], cval=255).astype(np.int64)
        return np.where(np.clip(hi - lo, 0, 255) > 24, 255, 0).astype(np.uint8)

    assert np.array_equal(CR.run(img, ps["edges"]), _per_channel(img, edges))
