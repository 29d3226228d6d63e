"""The numpy reference of the affine warp (``tests/_warp_ref.py``) against things that do not share its rule: numpy
indexing where the answer is exact, ``scipy.ndimage.affine_transform`` on linear ramps where it is not; and the
Python value ``Warp`` with its builders, which need no GPU.
"""
import numpy as np
import pytest

import _warp_ref as R
import vfilter
from vfilter import Warp, warps
from vfilter.filters import Chain, Combine, Invert

BORDERS = [R.REFLECT101, R.REPLICATE, R.CONSTANT]


def _frame(h, w, c, seed=0):
    return np.random.default_rng([h, w, c, seed]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)


def _reflect_by_turns(p, n):
    """Reflect-101 the slow way, a reflection at a time (no remainder)."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
def test_identity_and_flips(c, interp):
    for h, w in [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (23, 37)]:
        img = _frame(h, w, c)
        for border in BORDERS:
            assert np.array_equal(R.warp(img, [1, 0, 0, 0, 1, 0], interp=interp, border=border, value=(9, 8, 7)), img)
            assert np.array_equal(R.warp(img, mode=R.FLIP_H, interp=interp, border=border), img[:, ::-1])
            assert np.array_equal(R.warp(img, mode=R.FLIP_V, interp=interp, border=border), img[::-1])
            assert np.array_equal(R.warp(img, mode=R.FLIP_BOTH, interp=interp, border=border), img[::-1, ::-1])


@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
@pytest.mark.parametrize("dx,dy", [(1, 0), (0, 1), (3, 2), (-2, 5), (-4, -3), (2, -1)])
def test_whole_pixel_shifts_under_each_border(interp, dx, dy):
    """dst(y, x) = src(y - dy, x - dx): the map from destination to source subtracts the shift."""
    h, w = 11, 13
    for c in (1, 3):
        img = _frame(h, w, c, 1)
        m = [1, 0, -dx, 0, 1, -dy]
        ys, xs = np.arange(h) - dy, np.arange(w) - dx
        # constant: a zero-filled shifted copy
        want = np.zeros_like(img)
        yy, xx = np.arange(h)[(ys >= 0) & (ys < h)], np.arange(w)[(xs >= 0) & (xs < w)]
        want[np.ix_(yy, xx)] = img[np.ix_(yy - dy, xx - dx)]
        assert np.array_equal(R.warp(img, m, interp=interp, border=R.CONSTANT), want)
        fill = (17, 99, 201)
        want[...] = fill[:c] if c == 3 else fill[0]
        want[np.ix_(yy, xx)] = img[np.ix_(yy - dy, xx - dx)]
        assert np.array_equal(R.warp(img, m, interp=interp, border=R.CONSTANT, value=fill), want)
        # replicate: clipped indices
        want = img[np.ix_(np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1))]
        assert np.array_equal(R.warp(img, m, interp=interp, border=R.REPLICATE), want)
        # reflect-101: numpy's "reflect" pad
        pad = 6
        spec = ((pad, pad), (pad, pad)) + (((0, 0),) if c == 3 else ())
        padded = np.pad(img, spec, mode="reflect")
        want = padded[np.ix_(ys + pad, xs + pad)]
        assert np.array_equal(R.warp(img, m, interp=interp, border=R.REFLECT101), want)


@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
def test_a_shift_that_leaves_the_frame(interp):
    img = _frame(5, 7, 3, 2)
    for m in ([1, 0, 40, 0, 1, 0], [1, 0, 0, 0, 1, -40], [1, 0, -7, 0, 1, 5]):
        out = R.warp(img, m, interp=interp, border=R.CONSTANT, value=(1, 2, 3))
        assert np.array_equal(out, np.broadcast_to(np.array([1, 2, 3], np.uint8), img.shape))
    # one column short of leaving: the last source column is still read, unblended (a whole-pixel shift)
    out = R.warp(img, [1, 0, 6, 0, 1, 0], interp=interp, border=R.CONSTANT, value=(1, 2, 3))
    assert np.array_equal(out[:, 0], img[:, 6]) and np.all(out[:, 1:] == np.array([1, 2, 3], np.uint8))


@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_a_translation_near_a_million_saturates_the_coordinate(interp, n):
    """The fixed-point sum is far outside 16 bits; the coordinate is clamped to -32768 or 32767 and goes through
    the border rule from there."""
    for h, w in ((n, 4), (4, n), (n, n)):
        img = _frame(h, w, 1, 3)
        for tx, ty, sx, sy in ((999999, -999998, 32767, -32768), (-1000001, 3, -32768, None), (2, 1000000, None, 32767)):
            m = [1, 0, tx, 0, 1, ty]
            cols = [sx] * w if sx is not None else list(np.arange(w) + tx)
            rows = [sy] * h if sy is not None else list(np.arange(h) + ty)
            rep = img[np.ix_(np.clip(rows, 0, h - 1), np.clip(cols, 0, w - 1))]
            assert np.array_equal(R.warp(img, m, interp=interp, border=R.REPLICATE), rep)
            ref = img[np.ix_([_reflect_by_turns(int(p), h) for p in rows], [_reflect_by_turns(int(p), w) for p in cols])]
            assert np.array_equal(R.warp(img, m, interp=interp, border=R.REFLECT101), ref)
            assert np.all(R.warp(img, m, interp=interp, border=R.CONSTANT, value=77) == 77)


def test_the_border_index_against_turn_by_turn_reflection():
    for n in range(1, 10):
        p = np.arange(-400, 400)
        assert list(R.border_index(p, n, R.REFLECT101)) == [_reflect_by_turns(int(v), n) for v in p]
        assert list(R.border_index(p, n, R.REPLICATE)) == [min(max(int(v), 0), n - 1) for v in p]
        assert list(R.border_index(p, n, R.CONSTANT)) == [int(v) if 0 <= v < n else -1 for v in p]
    assert int(R.border_index(-32768, 2, R.REFLECT101)) == 0 and int(R.border_index(32767, 2, R.REFLECT101)) == 1


def test_a_constant_border_is_decided_tap_by_tap():
    """Half a pixel to the left of the frame: the first column blends the border colour and column 0 evenly."""
    img = np.full((3, 4), 200, np.uint8)
    out = R.warp(img, [1, 0, -0.5, 0, 1, 0], border=R.CONSTANT, value=100)
    assert np.all(out[:, 0] == 150) and np.all(out[:, 1:] == 200)
    out = R.warp(img, [1, 0, 0, 0, 1, 0.25], border=R.CONSTANT, value=0)
    assert np.all(out[:2] == 200) and np.all(out[2] == 150)


def test_linear_ramps_against_scipy():
    """On a ramp a x + b y + c bilinear interpolation is exact, so the warp is the ramp at the quantised coordinate,
    rounded: it differs from the ramp at the true coordinate by at most 0.5 + (|a| + |b|)(1 / 64 + 1 / 1024).  scipy
    computes the true one in float64; its own rounding gets the other half."""
    ndimage = pytest.importorskip("scipy.ndimage")
    h, w = 23, 37
    rng = np.random.default_rng(2024)
    ys, xs = np.mgrid[0:h, 0:w]
    done, worst = 0, 0.0
    while done < 80:
        a, b = (int(v) for v in rng.integers(-6, 7, 2))
        span = abs(a) * (w - 1) + abs(b) * (h - 1)
        if span > 255 or (a == 0 and b == 0):
            continue
        ramp = a * xs + b * ys
        ramp = ramp - ramp.min() + int(rng.integers(0, 256 - span))
        img = ramp.astype(np.uint8)
        assert np.array_equal(img, ramp)
        angle, scale = rng.uniform(-180, 180), rng.uniform(0.6, 1.8)
        fwd = R.rotation(((w - 1) / 2 + rng.uniform(-3, 3), (h - 1) / 2 + rng.uniform(-3, 3)), angle, scale)
        m = R.invert_affine(fwd)
        got = R.warp(img, m, interp=R.LINEAR, border=R.CONSTANT).astype(np.float64)
        # mode "nearest": a true coordinate may lie up to 1 / 64 + 1 / 1024 past the last column while the quantised
        # one is inside; scipy then reads the ramp at the edge, which is nearer to ours than the true one is
        want = ndimage.affine_transform(ramp.astype(np.float64), [[m[4], m[3]], [m[1], m[0]]], offset=[m[5], m[2]],
                                        order=1, mode="nearest")
        sx, sy, _, _ = R.coords(m, w, h, R.LINEAR)
        inside = (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)
        if inside.sum() < 20:
            continue
        bound = 1 + (abs(a) + abs(b)) * (1 / 64 + 1 / 1024)
        err = np.abs(got - want)[inside].max()
        worst = max(worst, err / bound)
        assert err <= bound, (a, b, angle, scale, err, bound)
        done += 1
    assert worst > 0.1  # the comparison is not vacuous: the quantisation shows


def test_the_inversion_is_cv2s_formula():
    fwd = warps.rotation((10.5, 7.25), 30.0, 1.3)
    assert np.array_equal(fwd, R.rotation((10.5, 7.25), 30.0, 1.3))
    f = Warp(fwd)
    assert f.m == tuple(R.invert_affine(fwd)) and f.mode == 0 and f.family == "warp"
    m = np.array(f.m).reshape(2, 3)
    full = np.vstack([fwd, [0, 0, 1]]) @ np.vstack([m, [0, 0, 1]])
    assert np.allclose(full, np.eye(3), atol=1e-12)
    assert Warp(fwd, inverse_map=True).m == tuple(float(v) for v in fwd.reshape(6))
    assert Warp([[1, 2, 3], [2, 4, 5]]).m == (0.0, -0.0, 0.0, -0.0, 0.0, 0.0)  # singular: D = 0, as cv2
    assert np.array_equal(warps.translation(3, -2), [[1, 0, 3], [0, 1, -2]])
    assert np.allclose(warps.zoom(2.0, (5, 5)), [[2, 0, -5], [0, 2, -5]])
    a = 1.3 * np.cos(np.pi / 6)
    assert np.isclose(fwd[0, 0], a) and np.isclose(fwd[1, 0], -1.3 * 0.5) and np.isclose(fwd[0, 2], (1 - a) * 10.5 - 0.65 * 7.25)


def test_the_value_and_its_refusals():
    f = Warp(flip="h")
    assert f.args == (None, 1, 0, 2, (0, 0, 0)) and Warp(flip=0).mode == 2 and Warp(flip=-1).mode == 3 and Warp(flip=1).mode == 1
    assert Warp(flip="both", interpolation="nearest", border="replicate", border_value=(1, 2, 3)).args == (None, 3, 1, 1, (1, 2, 3))
    assert Warp(warps.translation(1, 1), border_value=7).value == (7, 7, 7)
    with pytest.raises(dataclasses_error()):
        f.mode = 2
    for kw in (dict(), dict(matrix=np.eye(3)[:2], flip="h"), dict(flip="x"), dict(flip=2), dict(flip=True),
               dict(matrix=np.eye(3)), dict(matrix=[1, 2, 3]), dict(matrix=[[1, 0, np.nan], [0, 1, 0]]),
               dict(matrix=[[1, 0, np.inf], [0, 1, 0]]), dict(matrix="abc"),
               dict(flip="h", interpolation="cubic"), dict(flip="h", border="wrap"), dict(flip="h", border_value=256),
               dict(flip="h", border_value=-1), dict(flip="h", border_value=(1, 2)), dict(flip="h", border_value=1.5),
               dict(matrix=[[1e-160, 0, 1e200], [0, 1e-160, 0]])):
        with pytest.raises(ValueError):
            Warp(**kw)


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_a_warp_is_a_chain_step_and_the_entry_points_refuse_shape_changes():
    c = Chain([Warp(flip="h"), Invert()])
    assert c.steps[0][0] == 12 and c.steps[0][6] == 2 and c.steps[0][4] == ((0.0,) * 6, 1, 0, (0, 0, 0))
    c = Chain([Combine("absdiff", None, Warp(warps.translation(2, 0), border_value=0))])
    assert [s[0] for s in c.steps] == [12, 3]
    img = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="frames keep their size"):
        vfilter.warp_affine(img, warps.translation(1, 0), dsize=(4, 6))
    with pytest.raises(ValueError, match="frames keep their size"):
        vfilter.warp_affine(img, warps.translation(1, 0), dsize=(12, 8))
    for code in ("90_clockwise", "90_counterclockwise", 0, 2, True):
        with pytest.raises(ValueError, match="frames keep their size"):
            vfilter.rotate(img, code)
    with pytest.raises(ValueError, match="cubic"):
        vfilter.warp_affine(img, warps.translation(1, 0), flags=2)
    with pytest.raises(ValueError):
        vfilter.warp_frames([img], Invert())
    with pytest.raises(ValueError):
        vfilter.flip(img, "diagonal")
    with pytest.raises(ValueError, match="or a Clahe, not str"):
        Chain(["warp"])
    empty = np.empty((0, 0, 3), np.uint8)  # no GPU work for the empty frame
    assert vfilter.flip(empty, 1).shape == (0, 0, 3) and vfilter.warp_affine(empty, warps.translation(1, 1), dsize=(0, 0)).shape == (0, 0, 3)
