"""The convolution filter's host side without a GPU: ``vfilter.as_kernel`` (the dyadic rule and
the limits), the ready-made ``vfilter.kernels``, and the tests' own numpy reference
(``tests/_conv_ref.py``) -- against hand-computed corners and against a float32 evaluation, which
is what ``cv2.filter2D`` does (float32 kernel and sum, round to nearest even, saturate)."""
import numpy as np
import pytest

import _conv_ref as R
import vfilter
from vfilter import kernels as K


# ---- as_kernel -----------------------------------------------------------------------------

def test_integer_kernels_keep_their_weights():
    w, s = vfilter.as_kernel(np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]]))
    assert w.dtype == np.int16 and w.flags.c_contiguous and s == 0
    assert w.tolist() == [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]
    w, s = vfilter.as_kernel([[1, 2, 1]])  # a list; 3 wide x 1 high
    assert w.shape == (1, 3) and s == 0
    w, s = vfilter.as_kernel(np.array([[3.0]]))  # integral floats are integers
    assert w.tolist() == [[3]] and s == 0


def test_dyadic_float_kernels_get_the_smallest_shift():
    g = np.outer([1, 2, 1], [1, 2, 1]) / 16.0
    w, s = vfilter.as_kernel(g)
    assert s == 4 and w.tolist() == [[1, 2, 1], [2, 4, 2], [1, 2, 1]]
    w, s = vfilter.as_kernel(np.array([[0.5, 0.5, 1.0]], dtype=np.float32))
    assert s == 1 and w.tolist() == [[1, 1, 2]]
    w, s = vfilter.as_kernel(np.array([[2.0 ** -16]]))
    assert s == 16 and w.tolist() == [[1]]


def test_weights_and_shift_pairs_are_normalised():
    w, s = vfilter.as_kernel((np.array([[2, 4, 2]]), 3))
    assert s == 2 and w.tolist() == [[1, 2, 1]]
    w, s = vfilter.as_kernel((np.array([[1, 4, 2]]), 3))
    assert s == 3 and w.tolist() == [[1, 4, 2]]
    w, s = vfilter.as_kernel((np.array([[4]]), 1))  # 4 / 2 = 2: shift 0
    assert s == 0 and w.tolist() == [[2]]
    w, s = vfilter.as_kernel((np.zeros((3, 3), int), 5))
    assert s == 0 and not w.any()
    for name in ("gaussian3", "gaussian5", "gaussian7", "sobel_x"):
        pair = getattr(K, name)()
        w, s = vfilter.as_kernel(pair)
        assert s == pair[1] and np.array_equal(w, pair[0])


@pytest.mark.parametrize("bad", [
    np.full((3, 3), 1 / 9),                       # the 3 x 3 mean
    np.array([[0.1, 0.8, 0.1]]),
    np.exp(-np.arange(-1, 2) ** 2 / 2.0)[None, :] / np.exp(-np.arange(-1, 2) ** 2 / 2.0).sum(),  # a sampled Gaussian
    np.array([[2.0 ** -17]]),                     # dyadic, but past shift 16
    np.array([[1 / 3]], dtype=np.float32),
    np.array([[np.nan]]),
    np.ones((2, 2), int), np.ones((3, 4), int), np.ones((4, 3), int),   # even sides
    np.ones((9, 9), int), np.ones((1, 9), int),                          # above 7
    np.ones(3, int), np.ones((1, 3, 3), int), np.zeros((0, 3), int),     # not 2-D
    (np.ones((3, 3), int), 17), (np.ones((3, 3), int), -1), (np.ones((3, 3), int), 1.5),
    (np.full((3, 3), 0.5), 1),                    # a pair's weights are integers
    np.array([[65537]]), np.full((7, 7), 1338),   # sum|K| > 65536
    np.array([[40000]]),                          # does not fit 16 bits
    np.array([["a"]]),
])
def test_refused_kernels(bad):
    with pytest.raises(ValueError):
        vfilter.as_kernel(bad)


def test_the_limits_themselves_are_accepted():
    w, s = vfilter.as_kernel((np.array([[32767, 0, 32767], [0, 2, 0], [0, 0, 0]]), 16))
    assert int(np.abs(w.astype(int)).sum()) == 65536 and s == 16
    assert vfilter.as_kernel(np.ones((7, 7), int))[0].shape == (7, 7)
    assert vfilter.as_kernel(np.ones((7, 1), int))[0].shape == (7, 1)


def test_borders():
    from vfilter.filters import border_code
    assert [border_code(b) for b in ("reflect101", "replicate", "constant")] == [0, 1, 2]
    for bad in ("reflect", "wrap", None, 4):
        with pytest.raises(ValueError):
            border_code(bad)


# ---- vfilter.kernels -----------------------------------------------------------------------

def test_each_kernel_is_its_closed_form():
    assert K.identity()[0].tolist() == [[1]] and K.identity()[1] == 0
    assert K.box(1)[0].tolist() == [[1]] and K.box(1)[1] == 0
    for n in (0, 2, 3, 5, 7, 9):  # 1/9, 1/25, 1/49 are not dyadic
        with pytest.raises(ValueError):
            K.box(n)
    b3, b5, b7 = [1, 2, 1], [1, 4, 6, 4, 1], [1, 6, 15, 20, 15, 6, 1]
    for got, row, shift in ((K.gaussian3(), b3, 4), (K.gaussian5(), b5, 8), (K.gaussian7(), b7, 12)):
        assert np.array_equal(got[0], np.outer(row, row)) and got[1] == shift
        assert int(got[0].astype(int).sum()) == 1 << got[1]  # sums to 2^shift: flat areas are kept
        assert got[0].dtype == np.int16
    assert K.sharpen() [0].tolist() == [[0, -1, 0], [-1, 5, -1], [0, -1, 0]]
    assert K.laplacian()[0].tolist() == [[0, 1, 0], [1, -4, 1], [0, 1, 0]]
    assert K.sobel_x()[0].tolist() == [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]
    assert np.array_equal(K.sobel_y()[0], K.sobel_x()[0].T)
    assert K.emboss()[0].tolist() == [[-2, -1, 0], [-1, 1, 1], [0, 1, 2]]
    for k in (K.sharpen(), K.laplacian(), K.sobel_x(), K.sobel_y(), K.emboss()):
        assert k[1] == 0
    assert int(K.sharpen()[0].sum()) == 1 and int(K.laplacian()[0].sum()) == 0 and int(K.emboss()[0].sum()) == 1


@pytest.mark.parametrize("amount", [0, 0.25, 0.5, 1, 1.5, 2, 3])
def test_unsharp_is_identity_plus_amount_times_detail(amount):
    w, s = K.unsharp(amount)
    ident = np.zeros((3, 3))
    ident[1, 1] = 1
    g = np.outer([1, 2, 1], [1, 2, 1]) / 16.0
    assert np.array_equal(w / 2.0 ** s, (1 + amount) * ident - amount * g)
    assert vfilter.as_kernel((w, s))[1] == s  # already at its smallest shift
    assert int(w.astype(int).sum()) == 1 << s


def test_unsharp_refuses_other_amounts():
    for bad in (0.3, 1 / 3, -1):
        with pytest.raises(ValueError):
            K.unsharp(bad)


# ---- the reference itself --------------------------------------------------------------------

def test_the_reference_reproduces_a_hand_computed_corner():
    """src = [[10, 20, 30], [40, 50, 60], [70, 80, 90]], K = [[1, 2, 3], [4, 5, 6], [7, 8, 9]] (not
    symmetric: a flipped or transposed kernel gives other numbers), at the top-left corner."""
    src = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], dtype=np.uint8)
    k = np.arange(1, 10).reshape(3, 3)
    # reflect101: rows (-1, 0, 1) -> (1, 0, 1), columns the same: the window is
    #   50 40 50 / 20 10 20 / 50 40 50
    want = 1 * 50 + 2 * 40 + 3 * 50 + 4 * 20 + 5 * 10 + 6 * 20 + 7 * 50 + 8 * 40 + 9 * 50
    assert want == 1650 and R.accumulate(src, k, "reflect101")[0, 0] == want
    # replicate: 10 10 20 / 10 10 20 / 40 40 50
    want = 1 * 10 + 2 * 10 + 3 * 20 + 4 * 10 + 5 * 10 + 6 * 20 + 7 * 40 + 8 * 40 + 9 * 50
    assert want == 1350 and R.accumulate(src, k, "replicate")[0, 0] == want
    # constant: 0 0 0 / 0 10 20 / 0 40 50
    want = 5 * 10 + 6 * 20 + 8 * 40 + 9 * 50
    assert want == 940 and R.accumulate(src, k, "constant")[0, 0] == want
    # and the bottom-right corner under reflect101: 50 60 50 / 80 90 80 / 50 60 50
    want = 1 * 50 + 2 * 60 + 3 * 50 + 4 * 80 + 5 * 90 + 6 * 80 + 7 * 50 + 8 * 60 + 9 * 50
    assert R.accumulate(src, k, "reflect101")[2, 2] == want
    # shift 4 of 1650: 103.125 -> 103; of 1350: 84.375 -> 84; saturation of the unshifted sums
    assert R.filter2d(src, k, 4, "reflect101")[0, 0] == 103 and R.filter2d(src, k, 4, "replicate")[0, 0] == 84
    assert R.filter2d(src, k, 0, "constant")[0, 0] == 255


def test_the_reference_rounds_half_to_even_and_floors_negatives():
    acc = np.array([5, 6, 7, 10, 14, -5, -6, -7, -10, -2, 2, 0])
    #      / 4 =    1.25 1.5 1.75 2.5 3.5 -1.25 -1.5 -1.75 -2.5 -0.5 0.5 0
    assert R.round_shift(acc, 2).tolist() == [1, 2, 2, 2, 4, -1, -2, -2, -2, 0, 0, 0]
    assert R.round_shift(acc, 0).tolist() == acc.tolist()
    assert R.round_shift(np.array([1, 3, -1, -3]), 1).tolist() == [0, 2, 0, -2]


def test_the_reference_reflects_more_than_once():
    src = np.array([[10, 200]], dtype=np.uint8)  # a 2-pixel axis under a 7-tap kernel
    k = np.array([[1, 2, 4, 8, 16, 32, 64]])
    # x = 0: taps at -3..3 -> 1 0 1 0 1 0 1 (indices) -> 200 10 200 10 200 10 200
    want = (1 + 4 + 16 + 64) * 200 + (2 + 8 + 32) * 10
    assert R.accumulate(src, k, "reflect101")[0, 0] == want
    one = np.array([[7]], dtype=np.uint8)  # a 1-pixel axis: every index is 0
    assert R.accumulate(one, np.ones((7, 7), int), "reflect101")[0, 0] == 49 * 7
    assert R.accumulate(one, np.ones((7, 7), int), "constant")[0, 0] == 7


@pytest.mark.parametrize("border", ["reflect101", "replicate", "constant"])
def test_the_reference_is_the_float32_evaluation(border):
    """Under sum|K| <= 65536 every product and partial sum is an integer below 2^24 times 2^-shift:
    exact in float32 in any order, so rint(float32 sum) is the integer definition.  This is the
    argument for equality with cv2.filter2D (not installed here), pinned on the test kernels."""
    img = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    ks = dict(R.kernel_set())
    ks["gaussian7"] = (K.gaussian7()[0].astype(int), 12)
    ks["limit"] = (np.array([[32767, 0, 32767], [0, 2, 0], [0, 0, 0]]), 16)
    for name, (w, s) in ks.items():
        assert np.array_equal(R.filter2d(img, w, s, border), R.filter2d_float32(img, w, s, border)), name
        assert np.array_equal(R.filter2d(img[:2, :1], w, s, border), R.filter2d_float32(img[:2, :1], w, s, border)), name


def test_the_test_kernels_produce_ties_negatives_and_saturation():
    img = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    total = np.zeros(3, dtype=np.int64)
    for name, (w, s) in R.kernel_set().items():
        total += np.array(R.stats(img, w, s))
    assert (total >= 100).all(), total
