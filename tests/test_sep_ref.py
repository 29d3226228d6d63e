"""The numpy reference of the separable filter (``tests/_sep_ref.py``) against independent statements
of the same definition, and the parts of ``vfilter`` that need no GPU: ``as_taps``, ``Separable`` and
the tap builders.  CPU only."""
import numpy as np
import pytest

import _conv_ref as CR
import _sep_ref as R
import vfilter
from vfilter import Separable, as_taps
from vfilter import kernels as K

BORDERS = ["reflect101", "replicate", "constant"]
_IMG = np.random.default_rng(2024).integers(0, 256, (80, 360, 3), dtype=np.uint8)
ODD = list(range(1, 32, 2))
AREAS = sorted({w * h for w in ODD for h in ODD})


@pytest.mark.parametrize("border", BORDERS)
def test_the_accumulator_is_filter2d_of_the_outer_product(border):
    """By definition sep(kx, ky) is filter2D with outer(ky, kx): against ``_conv_ref.accumulate`` for
    sides up to 7, on frames smaller than the radius as well."""
    rng = np.random.default_rng(7)
    for kw, kh in [(1, 1), (3, 3), (7, 7), (1, 7), (7, 1), (5, 3), (3, 7)]:
        kx, ky = rng.integers(-9, 10, kw), rng.integers(-9, 10, kh)
        for h, w in [(1, 1), (2, 3), (9, 40), (33, 31)]:
            img = np.ascontiguousarray(_IMG[:h, :w])
            assert np.array_equal(R.accumulate(img, kx, ky, border), CR.accumulate(img, np.outer(ky, kx), border))
            gray = img[:, :, 1].copy()
            assert np.array_equal(R.accumulate(gray, kx, ky, border), CR.accumulate(gray, np.outer(ky, kx), border))
    img = np.ascontiguousarray(_IMG[:20, :30])
    k5 = np.array([1, 4, 6, 4, 1])
    assert np.array_equal(R.sep(img, k5, k5, 8, border=border), CR.filter2d(img, np.outer(k5, k5), 8, border))


@pytest.mark.parametrize("border,mode", [("reflect101", "mirror"), ("replicate", "nearest"), ("constant", "constant")])
def test_against_scipy_correlate1d_applied_twice(border, mode):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(31)
    kx, ky = rng.integers(-8, 9, 31), rng.integers(-8, 9, 31)
    for h, w in [(1, 1), (2, 3), (9, 40), (33, 31)]:
        img = np.ascontiguousarray(_IMG[:h, :w]).astype(np.int64)
        rows = ndi.correlate1d(img, kx, axis=1, mode=mode, cval=0)
        want = ndi.correlate1d(rows, ky, axis=0, mode=mode, cval=0)
        assert np.array_equal(R.accumulate(img.astype(np.uint8), kx, ky, border), want), (h, w)


def test_the_box_division_equals_the_float_products_cv2_uses():
    """cv2.blur multiplies the integer sum by a float or double 1 / area and rounds to nearest.  For
    all 123 odd areas and every sum 0 .. 255 * area, floor((2 s + d) / (2 d)) equals both."""
    assert len(AREAS) == 123
    for d in AREAS:
        s = np.arange(255 * d + 1, dtype=np.int64)
        q = (2 * s + d) // (2 * d)
        assert np.array_equal(q, np.rint(s * (1.0 / d)).astype(np.int64)), d
        f32 = np.rint(s.astype(np.float32) * np.float32(1.0 / d))
        assert np.array_equal(q, f32.astype(np.int64)), d
        assert q[-1] == 255 and not ((2 * s + d) % (2 * d) == 0).any()  # no sum sits on a tie


def test_the_test_kernels_exercise_ties_negatives_and_saturation():
    """On this content: ends9 has ties of both parities (1431 even, 1403 odd), rand31x31 at least 7 of
    each plus negative sums and saturated outputs, rand15x5 27 / 25 / 1975 / 4332."""
    img = np.ascontiguousarray(_IMG[:37, :53])
    ks = R.kernel_set()
    even, odd, _, _ = R.stats(img, *ks["ends9"])
    assert even >= 1 and odd >= 1, (even, odd)
    for name in ("rand31x31", "rand15x5"):
        st = R.stats(img, *ks[name])
        assert all(v >= 1 for v in st), (name, st)
    kx, ky, s = ks["ends9"]
    a, b = R.sep(img, kx, ky, s, rounding="half_even"), R.sep(img, kx, ky, s, rounding="half_up")
    acc = R.accumulate(img, kx, ky)
    floor_even = ((acc >> 1) & 1) == 0
    assert np.array_equal(a != b, ((acc & 1) == 1) & floor_even)  # exactly on the ties whose floor is even
    assert int((a != b).sum()) == even


def test_as_taps():
    t, s = as_taps([1, 2, 1])
    assert t.dtype == np.int16 and t.tolist() == [1, 2, 1] and s == 0
    assert as_taps((np.array([2, 4, 2]), 3))[1] == 2 and as_taps((np.array([2, 4, 2]), 3))[0].tolist() == [1, 2, 1]
    t, s = as_taps(np.array([0.25, 0.5, 0.25]))
    assert t.tolist() == [1, 2, 1] and s == 2
    assert as_taps(np.array([1.0, -2.0, 1.0]))[1] == 0
    assert as_taps(K.binomial_taps(9))[1] == 8
    for bad in ([[1, 2, 1]], [], [1, 2], np.ones(33), [0.3, 0.4, 0.3], [1, np.inf, 1], ([1, 2, 1], 17), ([1, 2, 1], -1),
                ([1, 2, 1], 1.5), ([0.5, 1, 0.5], 2), [1, 40000, 1], np.array(["a", "b", "c"])):
        with pytest.raises(ValueError):
            as_taps(bad)


def test_separable_validates_before_a_context_exists():
    s = Separable([1, 2, 1])
    assert s.family == "sep" and s.ky.tolist() == [1, 2, 1] and s.shift == 0 and s.divisor == 1
    assert not s.kx.flags.writeable and not s.ky.flags.writeable
    taps = np.array([1, 2, 1])
    s = Separable(taps, rounding="half_up", border="replicate")
    taps[0] = 99  # copied
    assert s.kx.tolist() == [1, 2, 1] and s.args[4:] == (1, 1)
    kx, ky, shift, divisor, rounding, border = Separable(K.binomial_taps(7), K.binomial_taps(5)).args  # the C order
    assert kx.size == 7 and ky.size == 5 and shift == 10 and divisor == 1 and rounding == 0 and border == 0
    assert Separable(([2, 4, 2], 2), ([2, 4, 2], 2), shift=3).shift == 5  # the shifts add; the smallest common one
    assert Separable(K.binomial_taps(9)).shift == 16
    assert Separable([1, 1, 1], divisor=9).divisor == 9
    for bad in (lambda: Separable(K.binomial_taps(9), shift=1),        # 17 bits
                lambda: Separable([1, 1, 1], divisor=4), lambda: Separable([1, 1, 1], divisor=0),
                lambda: Separable([1, 1, 1], divisor=1025), lambda: Separable([1, 1, 1], divisor=2.5),
                lambda: Separable(([1, 2, 1], 2), divisor=3),          # a shift together with a divisor
                lambda: Separable([1, 1, 1], shift=1, divisor=3),
                lambda: Separable([300] * 3, [300] * 3),               # sum|kx| * sum|ky| > 65536
                lambda: Separable([1, 2, 1], rounding="nearest"), lambda: Separable([1, 2, 1], border="wrap"),
                lambda: Separable([1, 2]), lambda: Separable([1, 2, 1], [[1]]), lambda: Separable(np.ones(33)),
                lambda: Separable(Separable([1])), lambda: Separable([1, 2, 1], shift=-1)):
        with pytest.raises(ValueError):
            bad()


def test_box_and_gaussian_builders():
    b = Separable.box(5)
    assert b.kx.tolist() == [1] * 5 and b.ky.tolist() == [1] * 5 and b.divisor == 25 and b.shift == 0
    b = Separable.box((7, 3), border="replicate")  # cv2's order: (width, height)
    assert b.kx.size == 7 and b.ky.size == 3 and b.divisor == 21 and b.border == "replicate"
    assert Separable.box(31).divisor == 961 and Separable.box(3, normalize=False).divisor == 1
    for bad in (4, (3, 4), (2, 2), 33, 0, (3,), "5", 2.5):
        with pytest.raises(ValueError):
            Separable.box(bad)
    g = Separable.gaussian(15, 2.5)
    assert g.shift == 16 and g.rounding == "half_up" and g.kx.tolist() == K.gaussian_taps(15, 2.5)[0].tolist()
    g = Separable.gaussian((5, 9), (1.0, 2.0), bits=7)
    assert g.kx.size == 5 and g.ky.size == 9 and g.shift == 14
    for bad in (lambda: Separable.gaussian(15, 2.5, bits=9), lambda: Separable.gaussian(14, 2.5),
                lambda: Separable.gaussian(15, 0), lambda: Separable.gaussian(15, -1.0)):
        with pytest.raises(ValueError):
            bad()


def test_gaussian_taps_sum_to_a_power_of_two_and_are_symmetric():
    for ksize in ODD:
        for sigma in (0.3, 0.8, 1.5, 2.5, 5.0, 40.0):
            for bits in (4, 8, 14):
                t, s = K.gaussian_taps(ksize, sigma, bits)
                assert s == bits and t.dtype == np.int16 and t.size == ksize
                assert int(t.sum()) == 1 << bits and np.array_equal(t, t[::-1]) and (t >= 0).all(), (ksize, sigma, bits)
    assert K.gaussian_taps(1, 1.0)[0].tolist() == [256]
    for bad in (lambda: K.gaussian_taps(4, 1.0), lambda: K.gaussian_taps(33, 1.0), lambda: K.gaussian_taps(5, 0.0),
                lambda: K.gaussian_taps(5, 1.0, 15), lambda: K.gaussian_taps(5, float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_binomial_taps():
    assert K.binomial_taps(1) == (np.array([1], np.int16), 0) or K.binomial_taps(1)[0].tolist() == [1]
    for n in (3, 5, 7):
        t, s = K.binomial_taps(n)
        w, ws = getattr(K, "gaussian%d" % n)()
        assert np.array_equal(np.outer(t, t), w) and 2 * s == ws
    assert K.binomial_taps(9)[0].tolist() == R.BINOMIAL9.tolist() and K.binomial_taps(9)[1] == 8
    for bad in (2, 11, 0, -3):
        with pytest.raises(ValueError):
            K.binomial_taps(bad)


def test_kernels_box_is_what_it_was():
    with pytest.raises(ValueError):
        K.box(3)
    assert K.box(1)[0].tolist() == [[1]]


def test_step_sep_is_7_and_a_separable_is_a_chain_step():
    from vfilter import _lib, filters
    assert filters.STEP_SEP == 7 and _lib.STEP_SEP == 7
    c = vfilter.Chain([Separable.box(5), filters.Invert()])
    kind, a, b, op, data, shift, border = c.steps[0]
    assert (kind, a, b, op, shift, border) == (7, 0, 0, 0, 0, 0) and data[2] == 25 and data[0].size == 5
    c = vfilter.Chain(vfilter.Combine("add", None, vfilter.Combine("subtract", None, Separable.box(15))))
    assert [st[0] for st in c.steps] == [7, 3, 3]
    with pytest.raises(ValueError, match="Separable"):
        vfilter.Chain([object()])
