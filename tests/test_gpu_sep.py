"""The separable filter on raw frames (``vf_sep_frames_host``, ``vf_sep_device``, ``vfilter.sep_filter2d``,
``blur``, ``box_filter``) against the numpy reference of ``tests/_sep_ref.py``.  Every comparison is
exact.

The kernel's output tile comes from ``vf_sep_tile``: 256 row bytes (85 pixels and a byte for C = 3)
by a number of rows that depends on the vertical tap count.  The three channels of every image
carry different content and the random taps are asymmetric on both axes, so a swapped channel, a
flipped kernel or swapped axes cannot pass.
"""
import ctypes
import os

import numpy as np
import pytest

import _conv_ref as CR
import _sep_ref as R
import vfilter
from vfilter import Separable, _lib
from vfilter import kernels as K

pytestmark = pytest.mark.gpu

BORDERS = ["reflect101", "replicate", "constant"]
KERNELS = R.kernel_set()
_IMG = np.random.default_rng(2025).integers(0, 256, (120, 540, 3), dtype=np.uint8)


def _tile(kw, kh):
    rb, rows = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.load_library().vf_sep_tile(kw, kh, ctypes.byref(rb), ctypes.byref(rows)) == _lib.VF_OK
    return rb.value, rows.value


def _img(h, w, c):
    """h x w x c out of one random image (the channels differ), contiguous."""
    a = np.ascontiguousarray(_IMG[:h, :w, :c])
    return a if c == 3 else a[:, :, 0].copy()


def _grid(kw, kh, c):
    """The issue's W x H grid for this tile, W in pixels of c channels."""
    rb, th = _tile(kw, kh)
    tw = rb // c
    ws = [1, 2, 5, 14, 15, 16, tw - 1, tw, tw + 1, 2 * tw + 5]
    hs = [1, 2, 3, 14, 15, 16, 17, th - 1, th, th + 1, 2 * th + 3]
    return ws, hs, tw, th


def _straddle(kw, kh, c):
    _, _, tw, th = _grid(kw, kh, c)
    return [(tw - 1, th - 1), (tw, th), (tw + 1, th + 1), (2 * tw + 5, 2 * th + 3), (1, 1), (2, 2), (1, th + 1), (tw + 1, 2)]


def _check(ctx, img, kx, ky, shift=0, divisor=1, rounding="half_even", border="reflect101"):
    got = vfilter.sep_filter2d(img, (kx, 0), (ky, 0), shift=shift, divisor=divisor, rounding=rounding, border=border, ctx=ctx)
    want = R.sep(img, kx, ky, shift, divisor, rounding, border)
    assert got.shape == want.shape and np.array_equal(got, want), (
        len(kx), len(ky), shift, divisor, rounding, border, img.shape, np.argwhere(got != want)[:5])


def test_vf_sep_tile():
    assert _tile(1, 1)[0] == 256 and _tile(31, 31)[0] == 256
    for kw, kh in ((1, 1), (31, 1), (1, 31), (15, 15)):
        assert _tile(kw, kh)[1] in (16, 24, 32)
    lib = _lib.load_library()
    rb, rows = ctypes.c_int(0), ctypes.c_int(0)
    for kw, kh in ((2, 3), (3, 33), (0, 1)):
        assert lib.vf_sep_tile(kw, kh, ctypes.byref(rb), ctypes.byref(rows)) == _lib.VF_E_INVALID


@pytest.mark.parametrize("border", BORDERS)
def test_shape_sweep_full_grid_31x31(vf_ctx, border):
    kx, ky, s = KERNELS["rand31x31"]
    for c in (1, 3):
        ws, hs, _, _ = _grid(31, 31, c)
        for w in ws:
            for h in hs:
                _check(vf_ctx, _img(h, w, c), kx, ky, s, border=border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kw,kh", [(1, 1), (3, 3), (1, 31), (31, 1), (9, 5), (5, 9), (15, 15)])
def test_shape_sweep_straddling(vf_ctx, kw, kh, border):
    kx, ky, s = R.rand_taps(kw, kh)
    for c in (1, 3):
        for w, h in _straddle(kw, kh, c):
            _check(vf_ctx, _img(h, w, c), kx, ky, s, border=border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("rounding", ["half_even", "half_up"])
def test_binomial9_at_shift_16(vf_ctx, rounding, border):
    for c in (1, 3):
        for w, h in _straddle(9, 9, c):
            _check(vf_ctx, _img(h, w, c), R.BINOMIAL9, R.BINOMIAL9, 16, rounding=rounding, border=border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", ["ends9", "rand15x5"])
def test_the_named_kernels_under_both_roundings(vf_ctx, name, border):
    kx, ky, s = KERNELS[name]
    for rounding in ("half_even", "half_up"):
        for c in (1, 3):
            for w, h in _straddle(len(kx), len(ky), c):
                _check(vf_ctx, _img(h, w, c), kx, ky, s, rounding=rounding, border=border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kw,kh", [(3, 3), (5, 9), (31, 31)])
def test_boxes(vf_ctx, kw, kh, border):
    for c in (1, 3):
        for w, h in _straddle(kw, kh, c):
            img = _img(h, w, c)
            got = vfilter.blur(img, (kw, kh), border=border, ctx=vf_ctx)
            assert np.array_equal(got, R.box(img, kw, kh, True, border)), (kw, kh, border, img.shape)
    img = _img(40, 100, 3)
    assert np.array_equal(vfilter.box_filter(img, (kw, kh), normalize=False, border=border, ctx=vf_ctx),
                          R.box(img, kw, kh, False, border))
    assert np.array_equal(vfilter.box_filter(img, (kw, kh), border=border, ctx=vf_ctx), R.box(img, kw, kh, True, border))


def test_every_divisor_class_on_a_ramp(vf_ctx):
    """Sums 0 .. 255 * d through the division, for a few divisors with taps that are not a box: the
    quotient's every step is crossed."""
    ramp = np.tile(np.arange(256, dtype=np.uint8), (3, 2))[:, :, None].repeat(3, axis=2).copy()
    for d, kx in ((3, [1, 1, 1]), (7, [2, 3, 2]), (1023, [341, 341, 341]), (961, [300, 361, 300]), (5, [-1, 7, -1])):
        _check(vf_ctx, ramp, np.array(kx), np.array([1]), divisor=d, border="replicate")
        _check(vf_ctx, ramp, np.array([1]), np.array(kx), divisor=d, border="replicate")


def _with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.mark.parametrize("border", BORDERS)
def test_the_sum_widths_agree(vf_ctx, border):
    """The vertical sums are int16 while 255 * sum|ky| < 2^15, i.e. sum|ky| <= 128; VF_SEP_FORM=wide, read
    per call, forces int32.  At 129 the 16-bit form cannot hold the sums: the result is exact anyway."""
    lim = np.array([-20, 30, -14, 10, 7, -9, -25, 5, 8])
    assert np.abs(lim).sum() == 128
    over = lim.copy()
    over[4] += 1
    kx = np.array([3, -1, 4, 1, -5])
    for ky in (lim, over, np.array([1, 2, 1])):
        for c in (1, 3):
            img = _img(40, 300, c)
            want = R.sep(img, kx, ky, 6, border=border)
            for form in ("wide", "narrow"):
                got = _with_env("VF_SEP_FORM", form, lambda: vfilter.sep_filter2d(img, kx, ky, shift=6, border=border, ctx=vf_ctx))
                assert np.array_equal(got, want), (ky.tolist(), c, form)


@pytest.mark.parametrize("rows", ["16", "24", "32"])
def test_every_tile_height_the_launcher_takes(vf_ctx, rows):
    """VF_SEP_ROWS overrides the plan's tile height where the LDS allows (a measurement's switch):
    every height gives the same bytes, and vf_sep_tile reports the height in use."""
    kx, ky, s = KERNELS["rand31x31"]
    for kxx, kyy, sh in ((kx, ky, s), (kx[:5], ky[:5], 5)):
        th = _with_env("VF_SEP_ROWS", rows, lambda: _tile(len(kxx), len(kyy))[1])
        assert th in (16, 24, 32)
        for c in (1, 3):
            img = _img(2 * th + 3, 300, c)
            got = _with_env("VF_SEP_ROWS", rows, lambda: vfilter.sep_filter2d(img, kxx, kyy, shift=sh, ctx=vf_ctx))
            assert np.array_equal(got, R.sep(img, kxx, kyy, sh)), (rows, th, c)


def test_agreement_with_filter2d(vf_ctx):
    """Wherever both exist the separable filter and filter2d with outer(ky, kx) give the same bytes."""
    img = _img(70, 300, 3)
    for n in (3, 5, 7):
        taps = K.binomial_taps(n)
        want = vfilter.filter2d(img, getattr(K, "gaussian%d" % n)(), ctx=vf_ctx)
        assert np.array_equal(vfilter.sep_filter2d(img, taps, taps, ctx=vf_ctx), want), n
        assert np.array_equal(want, CR.filter2d(img, np.outer(taps[0], taps[0]).astype(int), 2 * taps[1]))
    for name, kx, ky in (("sobel_x", [-1, 0, 1], [1, 2, 1]), ("sobel_y", [1, 2, 1], [-1, 0, 1])):
        want = vfilter.filter2d(img, getattr(K, name)(), ctx=vf_ctx)
        assert np.array_equal(vfilter.sep_filter2d(img, kx, ky, ctx=vf_ctx), want), name


@pytest.mark.parametrize("kw,kh", [(31, 31), (1, 31), (31, 1), (3, 3)])
@pytest.mark.parametrize("w,c", [(27, 3), (7, 3), (5, 3), (21, 1), (15, 1), (95, 1)])  # W * C mod 16 = 1, 5, 15
@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (1, 5)])
def test_row_pitch_and_pointers_off_the_16_byte_grid(vf_ctx, kw, kh, w, c, so, do):
    assert (w * c) % 16 in (1, 5, 15)
    h = _tile(kw, kh)[1] + 3
    img = _img(h, w, c)
    n = img.nbytes
    kx, ky, s = R.rand_taps(kw, kh)
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.sep_device(dsrc + so, ddst + 16 + do, w, h, c, kx.astype(np.int16), ky.astype(np.int16), s)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), R.sep(img, kx, ky, s))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)  # the canaries on both sides


@pytest.mark.parametrize("name", ["identity31", "rand31x31", "box15"])
def test_device_resident_multi_tile(vf_ctx, name):
    """(4 TW + 9) x (4 TH + 1) x 3: five tiles by five, the last column and row partial.  The identity
    of 31 taps, a 1 in the middle, isolates the halo staging: any slip of a row or a byte shows."""
    rb, th = _tile(31, 31)
    w, h = 4 * (rb // 3) + 9, 4 * th + 1
    img = _img(h, w, 3)
    ident = np.zeros(31, dtype=np.int64)
    ident[15] = 1
    kx, ky, s, d = {"identity31": (ident, ident, 0, 1), "rand31x31": KERNELS["rand31x31"] + (1,),
                    "box15": (np.ones(15, int), np.ones(31, int), 0, 465)}[name]
    got = np.empty_like(img)
    dsrc, ddst = vf_ctx.alloc_device(img.nbytes), vf_ctx.alloc_device(img.nbytes)
    try:
        vf_ctx.upload(dsrc, img, img.nbytes)
        vf_ctx.sep_device(dsrc, ddst, w, h, 3, kx.astype(np.int16), ky.astype(np.int16), s, d)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, img.nbytes)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    if name == "identity31":
        assert np.array_equal(got, img)
    assert np.array_equal(got, R.sep(img, kx, ky, s, d))


def _first_bad_row(got, want):
    rows = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    return "equal" if rows.size == 0 else "%d rows differ, the first is row %d, the last row %d" % (rows.size, rows[0], rows[-1])


@pytest.mark.parametrize("w,c", [(1, 3), (3, 1)])
def test_the_row_seam_of_a_launch(vf_ctx, w, c):
    """A launch is split at 65535 x 16 = 1,048,560 rows (the grid's y limit with the shortest tile), each
    part with its own first row and destination.  A frame of 1,048,577 rows of 3 bytes crosses the
    seam, and the 31 vertical taps of the second launch reach 15 rows back over it."""
    h = 65535 * 16 + 17
    img = np.random.default_rng([6, w, c]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)
    n = img.nbytes
    for kw, kh in ((3, 31), (1, 3)):
        kx, ky, s = R.rand_taps(kw, kh)
        want = R.sep(img, kx, ky, s)
        got = np.empty_like(img)
        dsrc, ddst = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n)
        try:
            vf_ctx.upload(dsrc, img, n)
            vf_ctx.sep_device(dsrc, ddst, w, h, c, kx.astype(np.int16), ky.astype(np.int16), s)
            vf_ctx.sync()
            vf_ctx.download(got, ddst, n)
            vf_ctx.sync()
        finally:
            vf_ctx.free_device(dsrc)
            vf_ctx.free_device(ddst)
        assert np.array_equal(got, want), (kw, kh, "device", _first_bad_row(got, want))
        got = vfilter.sep_filter2d(img, kx, ky, shift=s, ctx=vf_ctx)
        assert np.array_equal(got, want), (kw, kh, "host", _first_bad_row(got, want))


def test_bands_of_a_frame_larger_than_the_staging():
    """1024 x 700 x 3 in 1 MiB of staging, which holds 341 rows: with kh = 31 the bands are [0, 326),
    [326, 637), [637, 700), each uploaded with 15 rows of halo, the border resolved against the frame."""
    big = np.random.default_rng(12).integers(0, 256, (700, 1024, 3), dtype=np.uint8)
    kx, ky, s = KERNELS["rand31x31"]
    sep = Separable(kx, ky, shift=s)
    box = Separable.box((5, 31), border="replicate")
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        want = R.sep(big, kx, ky, s)
        got = vfilter.sep_filter2d(big, sep, ctx=ctx)
        assert np.array_equal(got, want), _first_bad_row(got, want)
        buf = big.copy()  # host src is dst: a band's halo rows are the band before's output
        ctx.sep_frames_host([buf], [buf], [1024], [700], 3, *box.args)
        want_box = R.box(big, 5, 31, True, "replicate")
        assert np.array_equal(buf, want_box), _first_bad_row(buf, want_box)
        frames = [big[:1, :1].copy(), big[:3, :5].copy(), big]  # a mixed batch
        outs = vfilter.sep_frames(frames, sep, ctx=ctx)
        for f, o in zip(frames, outs):
            assert o.shape == f.shape and np.array_equal(o, want if f is big else R.sep(f, kx, ky, s)), f.shape


def test_conveniences(vf_ctx):
    img = _img(37, 53, 3)
    t7 = K.binomial_taps(7)
    want = R.sep(img, t7[0], t7[0], 12)
    assert np.array_equal(vfilter.sep_filter2d(img, t7, ctx=vf_ctx), want)          # ky=None: kx
    assert np.array_equal(vfilter.sep_filter2d(img, t7[0] / 64.0, t7, ctx=vf_ctx), want)  # dyadic floats
    g = Separable.gaussian(15, 2.5)
    gt = K.gaussian_taps(15, 2.5)[0]
    assert np.array_equal(vfilter.sep_filter2d(img, g, ctx=vf_ctx), R.sep(img, gt, gt, 16, rounding="half_up"))
    view = img[:, :, 2]
    assert np.array_equal(vfilter.blur(view, 5, ctx=vf_ctx), R.box(view.copy(), 5, 5))
    assert np.array_equal(vfilter.blur(img, (3, 7), ctx=vf_ctx), R.box(img, 3, 7))
    dst = np.empty_like(img)
    assert vfilter.blur(img, 5, dst=dst, ctx=vf_ctx) is dst and np.array_equal(dst, R.box(img, 5, 5))
    with pytest.raises(ValueError):
        vfilter.blur(img, 5, dst=img, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.sep_filter2d(img, t7, dst=img, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.blur(img, 4, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.sep_filter2d(img, g, shift=3, ctx=vf_ctx)


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _img(9, 11, 3)
    dst = np.empty_like(img)
    pkx, pky, ps = R.rand_taps(9, 5)
    probe_want = R.sep(img, pkx, pky, ps)

    def still_works():
        assert np.array_equal(vfilter.sep_filter2d(img, pkx, pky, shift=ps, ctx=vf_ctx), probe_want)

    ones = np.ones(33, np.int16)
    big = np.full(3, 86, np.int16)  # (3 * 86)^2 = 66564 > 65536
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)

    def host(kx=ones, kw=3, ky=ones, kh=3, shift=0, divisor=1, rounding=0, border=0, channels=3, widths=wa, heights=ha):
        xp = kx.ctypes.data if kx is not None else None
        yp = ky.ctypes.data if ky is not None else None
        return lib.vf_sep_frames_host(vf_ctx.handle, sa, da, widths, heights, 1, channels, xp, kw, yp, kh, shift, divisor,
                                      rounding, border)

    refusals = [
        (dict(kx=None), b"NULL"), (dict(ky=None), b"NULL"),
        (dict(kw=2), b"odd"), (dict(kh=4), b"odd"), (dict(kw=33), b"at most 31"), (dict(kh=33), b"at most 31"), (dict(kw=0), b"odd"),
        (dict(kx=big, ky=big), b"65536"),
        (dict(shift=17), b"shift"), (dict(shift=-1), b"shift"),
        (dict(divisor=4), b"divisor"), (dict(divisor=0), b"divisor"), (dict(divisor=-3), b"divisor"), (dict(divisor=1025), b"divisor"),
        (dict(shift=2, divisor=9), b"together"),
        (dict(rounding=2), b"rounding"), (dict(rounding=-1), b"rounding"),
        (dict(border=3), b"border"), (dict(border=-1), b"border"),
        (dict(channels=2), b"channels"), (dict(channels=4), b"channels"),
        (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(heights=(ctypes.c_int * 1)(-9)), b"frame"),
    ]
    for kwargs, word in refusals:
        assert host(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        assert word in lib.vf_last_error(vf_ctx.handle)
        still_works()
    assert host() == _lib.VF_OK  # the same call with nothing wrong
    assert host(divisor=9) == _lib.VF_OK and np.array_equal(dst, R.box(img, 3, 3))
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, kx=ones, kw=3, ky=ones, kh=3, shift=0, divisor=1, rounding=0, border=0, channels=3,
                w=11, h=9):
            xp = kx.ctypes.data if kx is not None else None
            return lib.vf_sep_device(vf_ctx.handle, src, dstp, w, h, channels, xp, kw, ky.ctypes.data, kh, shift, divisor,
                                     rounding, border, None)

        for kwargs, word in [(dict(kw=2), b"odd"), (dict(kh=33), b"at most 31"), (dict(shift=17), b"shift"),
                             (dict(kx=big, ky=big), b"65536"), (dict(divisor=2), b"divisor"),
                             (dict(shift=1, divisor=3), b"together"), (dict(rounding=5), b"rounding"),
                             (dict(channels=2), b"channels"), (dict(border=7), b"border"), (dict(kx=None), b"NULL"),
                             (dict(w=0), b"frame"), (dict(dstp=d), b"overlap"), (dict(dstp=d + n - 1), b"overlap"),
                             (dict(src=None), b"NULL")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)

    # a VF_STEP_SEP step goes through the same checks
    step_data = np.array([1, 1, 1, 1, 1, 40000, 1], np.int32)  # ky[1] does not fit int16

    def chain(kind=7, data=step_data, kw=3, kh=3, shift=0, op=0, border=0):
        st = (_lib.Step * 1)()
        st[0].kind, st[0].a, st[0].op, st[0].kw, st[0].kh, st[0].shift, st[0].border = kind, 0, op, kw, kh, shift, border
        st[0].data = data.ctypes.data if data is not None else None
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, 3, st, 1)

    good = np.array([0, 1, 1, 1, 1, 1, 1], np.int32)  # divisor 0: none
    for kwargs, word in [(dict(), b"int16"), (dict(data=None), b"NULL"), (dict(data=good, kw=4), b"odd"),
                         (dict(data=good, shift=17), b"shift"), (dict(data=good, op=3), b"rounding"),
                         (dict(data=np.array([2, 1, 1, 1, 1, 1, 1], np.int32)), b"divisor"),
                         (dict(kind=6, data=good), b"unknown kind 6"), (dict(kind=4, data=good), b"unknown kind 4")]:
        assert chain(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        still_works()
    assert chain(data=good) == _lib.VF_OK and np.array_equal(dst, R.box(img, 3, 3, False))
    still_works()
