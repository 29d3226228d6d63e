"""The 2-D convolution filter on raw frames (``vf_conv_frames_host``, ``vf_conv_device``,
``vfilter.filter2d``) against the numpy reference of ``tests/_conv_ref.py``.  Every comparison
is exact.

The kernel's output tile is ``kTileBytes`` = 256 row bytes x ``kTileRows`` = 16 rows
(csrc/vf_tile_plan.h); a row is W * C bytes and tiles are cut in bytes, so for C = 3 a tile is 85
pixels and one byte of the 86th: TW = 85, TH = 16.  The kernel does not grid-stride (one
workgroup per tile).  The three channels of every image carry different content, and the kernel
set has an asymmetric 3 wide x 5 high member, so a swapped channel, a flipped or a transposed
kernel cannot pass.
"""
import ctypes
import os

import numpy as np
import pytest

import _conv_ref as R
import vfilter
from vfilter import _lib
from vfilter import kernels as K

pytestmark = pytest.mark.gpu

TW, TH = 85, 16
WS = [1, 2, 3, 4, 7, TW - 1, TW, TW + 1, 2 * TW + 5]
HS = [1, 2, 3, 6, TH - 1, TH, TH + 1, 2 * TH + 3]
BORDERS = ["reflect101", "replicate", "constant"]
KERNELS = R.kernel_set()
# shapes that straddle a tile in both directions, for every kernel; the whole grid for two of them
STRADDLE = [(TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 5, 2 * TH + 3), (1, 1), (2, 2), (1, TH + 1), (TW + 1, 2)]
FULL_GRID = ("random7", "random3x5")

_IMG = np.random.default_rng(2024).integers(0, 256, (80, 360, 3), dtype=np.uint8)


def _img(h, w, c):
    """h x w x c out of one random image (the channels differ), contiguous."""
    a = np.ascontiguousarray(_IMG[:h, :w, :c])
    return a if c == 3 else a[:, :, 0].copy()


def _check(ctx, img, name, border):
    w, s = KERNELS[name]
    got = vfilter.filter2d(img, (w, s), border=border, ctx=ctx)
    want = R.filter2d(img, w, s, border)
    assert got.shape == want.shape and np.array_equal(got, want), (name, border, img.shape, np.argwhere(got != want)[:5])


def test_the_reference_has_ties_negatives_and_saturation_on_this_content():
    img = _img(37, 53, 3)
    total = np.zeros(3, dtype=np.int64)
    for w, s in KERNELS.values():
        total += np.array(R.stats(img, w, s))
    assert (total >= 1).all(), total


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", list(KERNELS))
def test_shape_sweep(vf_ctx, name, border):
    shapes = [(w, h) for w in WS for h in HS] if name in FULL_GRID else STRADDLE
    for c in (1, 3):
        for w, h in shapes:
            _check(vf_ctx, _img(h, w, c), name, border)


@pytest.mark.parametrize("name", ["random7", "gaussian3"])
@pytest.mark.parametrize("w,c", [(27, 3), (7, 3), (5, 3), (21, 1), (15, 1), (95, 1)])  # W * C mod 16 = 1, 5, 15
@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (1, 5)])
def test_row_pitch_and_pointers_off_the_16_byte_grid(vf_ctx, name, w, c, so, do):
    assert (w * c) % 16 in (1, 5, 15)
    h = TH + 3
    img = _img(h, w, c)
    n = img.nbytes
    wts, s = vfilter.as_kernel(KERNELS[name])
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.conv_device(dsrc + so, ddst + 16 + do, w, h, c, wts, s, 0)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    lo = 16 + do
    want = R.filter2d(img, *KERNELS[name])
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), want)
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)  # the canaries on both sides


def _with_form(form, fn):
    old = os.environ.get("VF_CONV_FORM")
    os.environ["VF_CONV_FORM"] = form
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["VF_CONV_FORM"]
        else:
            os.environ["VF_CONV_FORM"] = old


@pytest.mark.parametrize("border", BORDERS)
def test_the_arithmetic_forms_agree(vf_ctx, border):
    """The narrow form (packed 16-bit) holds kernels with sum|K| * 255 < 2^15, i.e. sum|K| <= 128;
    VF_CONV_FORM, read per call, forces either form for such a kernel.  Both equal the reference.
    At 129 the narrow form cannot hold the kernel: whatever the switch says, the result is exact."""
    img = _img(2 * TH + 3, 2 * TW + 5, 3)
    lim = np.array([[-20, 30, -14], [10, 7, -9], [-25, 5, 8]])  # negatives: the 16-bit sums go below zero
    assert np.abs(lim).sum() == 128
    over = lim.copy()
    over[1, 1] += 1
    big5 = np.random.default_rng(3).integers(-5, 6, (5, 5))
    big7 = np.random.default_rng(4).integers(-2, 3, (7, 7))
    assert np.abs(big5).sum() <= 128 and np.abs(big7).sum() <= 128
    for w, s in [KERNELS["gaussian3"], KERNELS["sharpen"], KERNELS["sobel_x"], KERNELS["random3x5"], (lim, 3), (over, 3),
                 (big5, 2), (big7, 1)]:
        want = R.filter2d(img, w, s, border)
        outs = [_with_form(f, lambda: vfilter.filter2d(img, (w, s), border=border, ctx=vf_ctx)) for f in ("wide", "narrow")]
        outs.append(vfilter.filter2d(img, (w, s), border=border, ctx=vf_ctx))
        for o in outs:
            assert np.array_equal(o, want), (w.tolist(), s)
        gray = img[:, :, 1].copy()
        assert np.array_equal(_with_form("narrow", lambda: vfilter.filter2d(gray, (w, s), border=border, ctx=vf_ctx)),
                              R.filter2d(gray, w, s, border))


@pytest.mark.parametrize("name", ["identity", "gaussian5", "random7"])
def test_device_resident_multi_tile(vf_ctx, name):
    """(4 TW + 9) x (4 TH + 1) x 3: five tiles by five, the last column and row partial.  identity
    isolates the halo staging: any slip of a row or a byte shows."""
    w, h = 4 * TW + 9, 4 * TH + 1
    img = _img(h, w, 3)
    pair = (K.identity()[0].astype(int), 0) if name == "identity" else KERNELS[name]
    wts, s = vfilter.as_kernel(pair)
    got = np.empty_like(img)
    dsrc, ddst = vf_ctx.alloc_device(img.nbytes), vf_ctx.alloc_device(img.nbytes)
    try:
        vf_ctx.upload(dsrc, img, img.nbytes)
        vf_ctx.conv_device(dsrc, ddst, w, h, 3, wts, s, 0)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, img.nbytes)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    if name == "identity":
        assert np.array_equal(got, img)
    assert np.array_equal(got, R.filter2d(img, *pair))


def test_bands_of_a_frame_larger_than_the_staging():
    """max_frame_bytes = 1 MiB holds 182 rows of a 1080p frame: seven bands, each uploaded with its
    halo, the border resolved against the frame and not the band."""
    big = np.random.default_rng(8).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    w7, s7 = KERNELS["random7"]
    frames = [big[:1, :1].copy(), big[:3, :5].copy(), big[:480, :640].copy(), big]
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        want_big = R.filter2d(big, w7, s7, "reflect101")  # once: the reference is the slow side
        got = vfilter.filter2d(big, (w7, s7), border="reflect101", ctx=ctx)
        assert np.array_equal(got, want_big)
        outs = vfilter.filter2d_frames(frames, (w7, s7), ctx=ctx)  # a mixed batch: (1,1) (5,3) (640,480) (1920,1080)
        for f, o in zip(frames, outs):
            assert o.shape == f.shape and np.array_equal(o, want_big if f is big else R.filter2d(f, w7, s7)), f.shape
        # host src is dst, on a frame of three bands: a band's halo rows are the band before's output
        buf = big[:400].copy()
        want = R.filter2d(buf, w7, s7, "replicate")
        wts, s = vfilter.as_kernel((w7, s7))
        ctx.conv_frames_host([buf], [buf], [1920], [400], 3, wts, s, 1)
        assert np.array_equal(buf, want)


def test_filter2d_conveniences(vf_ctx):
    img = _img(37, 53, 3)
    g3 = KERNELS["gaussian3"]
    want = R.filter2d(img, *g3)
    assert np.array_equal(vfilter.filter2d(img, K.gaussian3(), ctx=vf_ctx), want)
    # a dyadic float kernel is its integer form
    assert np.array_equal(vfilter.filter2d(img, np.outer([1, 2, 1], [1, 2, 1]) / 16.0, ctx=vf_ctx), want)
    assert np.array_equal(vfilter.filter2d(img, np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float32), ctx=vf_ctx),
                          R.filter2d(img, *KERNELS["sharpen"]))
    # an H x W view (non-contiguous) and a plain H x W array
    view = img[:, :, 2]
    assert not view.flags.c_contiguous
    assert np.array_equal(vfilter.filter2d(view, g3, ctx=vf_ctx), R.filter2d(view.copy(), *g3))
    flipped = img[::-1, ::2]
    assert np.array_equal(vfilter.filter2d(flipped, g3, ctx=vf_ctx), R.filter2d(np.ascontiguousarray(flipped), *g3))
    # dst: filled and returned; refused when it has another shape, dtype or layout
    dst = np.empty_like(img)
    assert vfilter.filter2d(img, g3, dst=dst, ctx=vf_ctx) is dst and np.array_equal(dst, want)
    for bad in (np.empty((37, 53), np.uint8), np.empty(img.shape, np.int8), np.empty((53, 37, 3), np.uint8).transpose(1, 0, 2)):
        with pytest.raises(ValueError):
            vfilter.filter2d(img, g3, dst=bad, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.filter2d(img.astype(np.float32), g3, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.filter2d(img, np.full((3, 3), 1 / 9), ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.filter2d(img, g3, border="wrap", ctx=vf_ctx)
    for border in BORDERS:
        assert np.array_equal(vfilter.filter2d(img, K.sobel_y(), border=border, ctx=vf_ctx),
                              R.filter2d(img, K.sobel_y()[0].astype(int), 0, border))


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _img(9, 11, 3)
    dst = np.empty_like(img)
    probe_want = R.filter2d(img, *KERNELS["random3x5"])

    def still_works():
        assert np.array_equal(vfilter.filter2d(img, KERNELS["random3x5"], ctx=vf_ctx), probe_want)

    ones = np.ones(81, np.int16)
    big = np.full(9, 7282, np.int16)  # 9 * 7282 = 65538 > 65536
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)

    def host(weights=ones, kw=3, kh=3, shift=0, border=0, channels=3, widths=wa, heights=ha):
        wp = weights.ctypes.data if weights is not None else None
        return lib.vf_conv_frames_host(vf_ctx.handle, sa, da, widths, heights, 1, channels, wp, kw, kh, shift, border)

    refusals = [
        (dict(kw=2), b"kernel"), (dict(kh=4), b"kernel"), (dict(kw=9, kh=9), b"kernel"), (dict(kw=0), b"kernel"),
        (dict(shift=17), b"shift"), (dict(shift=-1), b"shift"),
        (dict(weights=big), b"65536"),
        (dict(channels=2), b"channels"), (dict(channels=4), b"channels"),
        (dict(border=3), b"border"), (dict(border=-1), b"border"),
        (dict(weights=None), b"weights is NULL"),
        (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(heights=(ctypes.c_int * 1)(-9)), b"frame"),
    ]
    for kwargs, word in refusals:
        assert host(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        assert word in lib.vf_last_error(vf_ctx.handle)
        still_works()
    assert host() == _lib.VF_OK  # the same call with nothing wrong
    # an empty batch and an empty frame do nothing
    assert lib.vf_conv_frames_host(vf_ctx.handle, None, None, None, None, 0, 3, ones.ctypes.data, 3, 3, 0, 0) == _lib.VF_OK
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, weights=ones, kw=3, kh=3, shift=0, border=0, channels=3, w=11, h=9):
            wp = weights.ctypes.data if weights is not None else None
            return lib.vf_conv_device(vf_ctx.handle, src, dstp, w, h, channels, wp, kw, kh, shift, border, None)

        for kwargs, word in [(dict(kw=2), b"kernel"), (dict(kw=9), b"kernel"), (dict(shift=17), b"shift"),
                             (dict(weights=big), b"65536"), (dict(channels=2), b"channels"), (dict(border=7), b"border"),
                             (dict(weights=None), b"weights is NULL"), (dict(w=0), b"frame"), (dict(h=-1), b"frame"),
                             (dict(dstp=d), b"overlap"), (dict(dstp=d + n - 1), b"overlap"), (dict(src=d + 1, dstp=d), b"overlap"),
                             (dict(src=None), b"NULL")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    still_works()


# ---- kernels that are not square ------------------------------------------------------------------
# The GPU kernel is compiled for the 3, 5 or 7 square that holds the kernel: a 1 x 7 kernel runs as
# 7 x 7 with six rows of zero weights, and stages R = 3 halo rows that a band of vertical radius 0
# does not hold.

OBLONG = R.oblong_set()


def _first_bad_row(got, want):
    """Where two frames differ, by row: for messages."""
    rows = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    return "equal" if rows.size == 0 else "%d rows differ, the first is row %d, the last row %d" % (rows.size, rows[0], rows[-1])


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", list(OBLONG))
def test_oblong_kernels_on_straddling_shapes(vf_ctx, name, border):
    k, s = OBLONG[name]
    for c in (1, 3):
        for w, h in STRADDLE:
            img = _img(h, w, c)
            got = vfilter.filter2d(img, (k, s), border=border, ctx=vf_ctx)
            want = R.filter2d(img, k, s, border)
            assert np.array_equal(got, want), (name, border, img.shape, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("name", ["1x7", "7x1"])
@pytest.mark.parametrize("w,c", [(27, 3), (7, 3), (5, 3), (21, 1), (15, 1), (95, 1)])  # W * C mod 16 = 1, 5, 15
@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (1, 5)])
def test_oblong_kernels_off_the_16_byte_grid(vf_ctx, name, w, c, so, do):
    h = TH + 3
    img = _img(h, w, c)
    n = img.nbytes
    wts, s = vfilter.as_kernel(OBLONG[name])
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.conv_device(dsrc + so, ddst + 16 + do, w, h, c, wts, s, 0)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), R.filter2d(img, *OBLONG[name]))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)  # the canaries on both sides


@pytest.mark.parametrize("name", ["1x7", "7x1"])
def test_bands_of_an_oblong_kernel(name):
    """1024 x 700 x 3 in 1 MiB of staging, which holds 341 rows.  1 x 7 has ry = 0: the bands are rows
    [0, 341), [341, 682), [682, 700) with no halo, and in place nothing is saved, yet the kernel
    (compiled as 7 x 7) stages three rows above and below that the band does not hold.  7 x 1 has
    ry = 3: bands [0, 338), [338, 673), [673, 700), each uploaded from three rows above."""
    big = np.random.default_rng(11).integers(0, 256, (700, 1024, 3), dtype=np.uint8)
    k, s = OBLONG[name]
    wts, sh = vfilter.as_kernel((k, s))
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for border in ("reflect101", "constant"):
            want = R.filter2d(big, k, s, border)
            got = vfilter.filter2d(big, (k, s), border=border, ctx=ctx)
            assert np.array_equal(got, want), (name, border, _first_bad_row(got, want))
            buf = big.copy()  # host src is dst
            ctx.conv_frames_host([buf], [buf], [1024], [700], 3, wts, sh, BORDERS.index(border))
            assert np.array_equal(buf, want), (name, border, "in place", _first_bad_row(buf, want))


@pytest.mark.parametrize("w,c", [(1, 3), (3, 1)])
def test_the_row_seam_of_a_launch(vf_ctx, w, c):
    """A launch is split at 65535 x 16 = 1,048,560 rows (the grid's y limit), each part with its own
    first row and destination.  A frame of 1,048,577 rows of 3 bytes crosses the seam: the second
    launch makes rows 1,048,560 to 1,048,576 and its taps reach back over the seam."""
    h = 65535 * TH + 17
    assert h == 1048577
    img = np.random.default_rng([5, w, c]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)
    n = img.nbytes
    for name, pair in (("gaussian3", KERNELS["gaussian3"]), ("7x1", OBLONG["7x1"])):
        want = R.filter2d(img, *pair)
        wts, s = vfilter.as_kernel(pair)
        got = np.empty_like(img)
        dsrc, ddst = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n)
        try:
            vf_ctx.upload(dsrc, img, n)
            vf_ctx.conv_device(dsrc, ddst, w, h, c, wts, s, 0)
            vf_ctx.sync()
            vf_ctx.download(got, ddst, n)
            vf_ctx.sync()
        finally:
            vf_ctx.free_device(dsrc)
            vf_ctx.free_device(ddst)
        assert np.array_equal(got, want), (name, "device", _first_bad_row(got, want))
        got = vfilter.filter2d(img, pair, ctx=vf_ctx)
        assert np.array_equal(got, want), (name, "host", _first_bad_row(got, want))
