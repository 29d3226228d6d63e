"""``_resize_ref`` against things that do not share its rule: slicing, ``np.repeat``, exact block means, exact
bilinear interpolation in float64 (and ``scipy.ndimage.zoom`` where scipy is present).  No pixel is exempt from
any check.

The linear bound of 1.5 is derived, not fitted: the two weights of a pass are rounded to 1 / 2048, which moves
a pass's value by at most 255 * 2 * 2^-12 (0.125, so about 0.25 over the two passes); ``>> 4`` drops under
2^-7 of a grey level from each horizontal value; the two ``>> 16`` drop under 0.25 each (under 0.5 together),
and the final ``(+ 2) >> 2`` rounds by at most 0.5.  The sum is below 1.26.
"""
import numpy as np
import pytest

import _resize_ref as R

MODES = (R.NEAREST, R.LINEAR, R.AREA)


def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5) % 256).astype(np.uint8)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), ramp]


@pytest.mark.parametrize("interp", MODES)
def test_identity(interp):
    for img in _frames(13, 7, 1) + _frames(1, 1, 2) + _frames(1, 9, 3):
        h, w = img.shape[:2]
        assert np.array_equal(R.resize(img, (w, h), interp=interp), img)
        assert np.array_equal(R.resize(img, None, 1.0, 1.0, interp), img)


@pytest.mark.parametrize("interp", MODES)
def test_a_constant_frame_stays_constant(interp):
    for v in (0, 1, 127, 254, 255):
        img = np.full((12, 24, 3), v, np.uint8)
        for dsize in [(24, 12), (12, 6), (8, 4), (6, 3), (2, 1)] + ([] if interp == R.AREA else [(31, 17), (5, 29), (48, 24), (1, 1)]):
            out = R.resize(img, dsize, interp=interp)
            assert out.shape == (dsize[1], dsize[0], 3) and np.all(out == v), (v, dsize)


def test_nearest_by_an_integer_is_a_slice_or_a_repeat():
    for img in _frames(24, 18, 4):
        h, w = img.shape[:2]
        for k in (1, 2, 3, 6):
            assert np.array_equal(R.resize(img, (w // k, h // k), interp=R.NEAREST), img[::k, ::k])
            up = np.repeat(np.repeat(img, k, axis=0), k, axis=1)
            assert np.array_equal(R.resize(img, (w * k, h * k), interp=R.NEAREST), up)


AREA_FACTORS = [(1, 1), (2, 2), (3, 2), (2, 3), (3, 3), (4, 4), (7, 5), (16, 16), (15, 16), (1, 4)]


@pytest.mark.parametrize("k,l", AREA_FACTORS)
def test_area_is_the_block_mean(k, l):
    for img in _frames(9 * k, 5 * l, 5):
        out = R.resize(img, (9, 5), interp=R.AREA).astype(np.float64)
        p = img.reshape(5, l, 9, k, -1).astype(np.int64).sum(axis=(1, 3))
        exact = p.reshape(out.shape) / float(k * l)
        # the float product's relative error is below 2^-22 on values of at most 255: 2^-13 covers it
        assert np.max(np.abs(out - exact)) <= 0.5 + 2.0 ** -13
        if (k, l) == (2, 2):
            assert np.array_equal(out.astype(np.int64), ((p + 2) >> 2).reshape(out.shape))


def _exact_bilinear(img, dw, dh):
    """Bilinear interpolation in float64 at cv2's sample positions, edges replicated."""
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.float64)
    h, w, _ = src.shape

    def axis(n_dst, n_src):
        pos = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
        i = np.floor(pos)
        return np.clip(i, 0, n_src - 1).astype(int), np.clip(i + 1, 0, n_src - 1).astype(int), pos - i

    x0, x1, fx = axis(dw, w)
    y0, y1, fy = axis(dh, h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return (top * (1 - fy) + bot * fy).reshape((dh, dw) + img.shape[2:])


LINEAR_PAIRS = [((7, 5), (20, 13)), ((20, 13), (7, 5)), ((16, 16), (17, 15)), ((33, 9), (100, 50)), ((100, 50), (33, 9)),
                ((5, 3), (1, 1)), ((1, 1), (5, 3)), ((9, 1), (4, 1)), ((1, 9), (1, 20)), ((40, 30), (39, 31)),
                ((12, 10), (36, 40)), ((64, 48), (21, 11))]


@pytest.mark.parametrize("size,dsize", LINEAR_PAIRS)
def test_linear_is_within_its_derived_bound_of_exact_bilinear(size, dsize):
    for img in _frames(size[0], size[1], 6):
        mode = R.resolve(size[0], size[1], dsize, interp=R.LINEAR)[0]
        assert mode == R.LINEAR
        out = R.resize(img, dsize, interp=R.LINEAR).astype(np.float64)
        assert np.max(np.abs(out - _exact_bilinear(img, dsize[0], dsize[1]))) <= 1.5


@pytest.mark.parametrize("size,dsize", LINEAR_PAIRS)
def test_exact_bilinear_is_scipys_zoom(size, dsize):
    ndimage = pytest.importorskip("scipy.ndimage")
    img = _frames(size[0], size[1], 7)[0].astype(np.float64)
    zoom = (dsize[1] / size[1], dsize[0] / size[0])
    z = ndimage.zoom(img, zoom, order=1, grid_mode=True, mode="nearest")
    assert z.shape == (dsize[1], dsize[0])
    assert np.max(np.abs(z - _exact_bilinear(img, dsize[0], dsize[1]))) <= 1e-9


def test_out_size_rounds_half_to_even():
    assert R.out_size(5, 5, None, 0.5, 0.5) == (2, 2)
    assert R.out_size(7, 7, None, 0.5, 0.5) == (4, 4)
    assert R.out_size(67, 35, None, 0.3, 0.3) == (20, 10)  # 20.1 and 10.5
    assert R.out_size(3, 3, None, 0.1, 0.1) == (0, 0)
    with pytest.raises(ValueError):
        R.resize(np.zeros((3, 3), np.uint8), None, 0.1, 0.1)


def test_the_fx_form_scales_by_one_over_fx():
    sx, sy = R.scales(7, 7, None, 0.5, 0.5)
    assert (sx, sy) == (2.0, 2.0)  # not 7 / 4
    img = _frames(7, 5, 8)[1]
    out = R.resize(img, None, 0.5, 0.5, R.AREA)  # 4 x 2: the last column's and the last row's blocks overrun
    assert out.shape == (2, 4, 3)
    s = img.astype(np.int64)
    assert np.array_equal(out[0, 0], (s[0:2, 0:2].sum(axis=(0, 1)) + 2) >> 2)          # a whole block
    assert np.array_equal(out[0, 3], np.rint(s[0:2, 6:7].sum(axis=(0, 1)) / 2.0))      # one column left: over its count
    assert np.all(np.abs(out[1, 0] - s[2:4, 0:2].sum(axis=(0, 1)) / 4.0) <= 0.5)       # rows 2 and 3 are whole


def test_linear_runs_as_area_at_exactly_two_by_two():
    img = _frames(12, 12, 9)[0]
    assert R.resolve(12, 12, (6, 6), interp=R.LINEAR)[0] == R.AREA
    assert np.array_equal(R.resize(img, (6, 6), interp=R.LINEAR), R.resize(img, (6, 6), interp=R.AREA))
    assert R.resolve(12, 12, (6, 4), interp=R.LINEAR)[0] == R.LINEAR  # 2 x 3
    assert R.resolve(12, 12, (4, 4), interp=R.LINEAR)[0] == R.LINEAR  # 3 x 3
    assert R.resolve(12, 12, None, 0.5, 0.5, R.LINEAR)[0] == R.AREA
    assert not np.array_equal(R.resize(img, (6, 4), interp=R.LINEAR), R.resize(img, (6, 4), interp=R.AREA))


def test_area_at_other_scales_is_refused():
    for dsize in [(8, 12), (18, 12), (12, 24)]:  # 1.5 x, an upscale on x, an upscale on y
        with pytest.raises(ValueError):
            R.resolve(12, 12, dsize, interp=R.AREA)
    with pytest.raises(ValueError):
        R.resolve(34, 34, (2, 2), interp=R.AREA)  # 17 x 17


def test_cv2s_integer_test_over_every_multiple():
    """1 / (dw / W) for W = k dw: DESIGN.md 26.1 records that every pair passes cv2's test with rint = k."""
    failed = []
    for k in range(1, 17):
        dw = np.arange(1, 2049, dtype=np.float64)
        scale = np.float64(1.0) / (dw / (dw * k))
        bad = np.flatnonzero(~(np.abs(scale - np.rint(scale)) < R.DBL_EPSILON) | (np.rint(scale) != k))
        failed += [(k, int(dw[i])) for i in bad]
    assert failed == []
