"""The rank filters on raw frames (``vf_rank_frames_host``, ``vf_rank_device``, ``vfilter.erode``,
``dilate``, ``median_blur``, ``rank_frames``) against the numpy reference of ``tests/_rank_ref.py``.
Every comparison is exact.

The kernel keeps the convolution's geometry: its output tile is ``kTileBytes`` = 256 row bytes
x ``kTileRows`` = 16 rows (csrc/vf_tile_plan.h); a row is W * C bytes and tiles are cut in
bytes, so for C = 3 a tile is 85 pixels and one byte of the 86th: TW = 85, TH = 16.  One
workgroup per tile, no grid stride.  The channels of every image carry different content; a
second image holds only the values {0, 1, 2, 3, 252, 253, 254, 255}, so equal values and both
extremes occur in every window.  random7 (centre not a member) and corner5 (only the top-left
corner) make a flip, a transpose or a wrong anchor fail and leave the set empty near an edge.
"""
import ctypes

import numpy as np
import pytest

import _rank_ref as R
import vfilter
from vfilter import Rank, _lib, elements

pytestmark = pytest.mark.gpu

TW, TH = 85, 16
WS = [1, 2, 3, 4, 7, TW - 1, TW, TW + 1, 2 * TW + 5]
HS = [1, 2, 3, 6, TH - 1, TH, TH + 1, 2 * TH + 3]
BORDERS = list(R.BORDERS)
ELEMENTS = R.element_set()
# shapes that straddle a tile in both directions (test_gpu_conv.py's subset)
STRADDLE = [(TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 5, 2 * TH + 3), (1, 1), (2, 2), (1, TH + 1), (TW + 1, 2)]
GRID = [(w, h) for w in WS for h in HS]

_IMG = np.random.default_rng(2025).integers(0, 256, (80, 360, 3), dtype=np.uint8)
_EXT = np.random.default_rng(2026).choice(np.array([0, 1, 2, 3, 252, 253, 254, 255], np.uint8), (80, 360, 3))


def _img(h, w, c, base=_IMG):
    """h x w x c out of one random image (the channels differ), contiguous."""
    a = np.ascontiguousarray(base[:h, :w, :c])
    return a if c == 3 else a[:, :, 0].copy()


def _run(ctx, img, op, arg, border):
    if op == "median":
        return vfilter.median_blur(img, arg, ctx=ctx)
    return (vfilter.erode if op == "erode" else vfilter.dilate)(img, arg, border=border, ctx=ctx)


def _check(ctx, img, op, arg, border="constant"):
    got = _run(ctx, img, op, arg, border)
    want = R.apply(img, op, arg, border)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (op, border, img.shape, np.argwhere(got != want)[:5])


def _sweep(ctx, shapes, op, arg, border="constant"):
    for c in (1, 3):
        for w, h in shapes:
            _check(ctx, _img(h, w, c), op, arg, border)
    for w, h in STRADDLE:  # ties and both extremes in every window
        _check(ctx, _img(h, w, 3, _EXT), op, arg, border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("op", ["erode", "dilate"])
def test_full_grid_random7(vf_ctx, op, border):
    _sweep(vf_ctx, GRID, op, ELEMENTS["random7"], border)


def test_full_grid_median5(vf_ctx):
    _sweep(vf_ctx, GRID, "median", 5)


def test_straddling_shapes_median3(vf_ctx):
    _sweep(vf_ctx, STRADDLE, "median", 3)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", [n for n in ELEMENTS if n != "random7"])
@pytest.mark.parametrize("op", ["erode", "dilate"])
def test_straddling_shapes(vf_ctx, op, name, border):
    _sweep(vf_ctx, STRADDLE, op, ELEMENTS[name], border)


@pytest.mark.parametrize("op,arg", [("median", 5), ("dilate", "random7")])
@pytest.mark.parametrize("w,c", [(27, 3), (7, 3), (5, 3), (21, 1), (15, 1), (95, 1)])  # W * C mod 16 = 1, 5, 15
@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (1, 5)])
def test_row_pitch_and_pointers_off_the_16_byte_grid(vf_ctx, op, arg, w, c, so, do):
    assert (w * c) % 16 in (1, 5, 15)
    h = TH + 3
    img = _img(h, w, c)
    n = img.nbytes
    rank = Rank.median(arg) if op == "median" else Rank.dilate(ELEMENTS[arg])
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.rank_device(dsrc + so, ddst + 16 + do, w, h, c, *rank.args)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    lo = 16 + do
    want = R.apply(img, op, rank.element.shape[0] if op == "median" else ELEMENTS[arg])
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), want)
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)  # the canaries on both sides


@pytest.mark.parametrize("name", ["identity", "erode_rect7", "median3"])
def test_device_resident_multi_tile(vf_ctx, name):
    """(4 TW + 9) x (4 TH + 1) x 3: five tiles by five, the last column and row partial.  The 1 x 1
    element isolates the halo staging: any slip of a row or a byte shows."""
    w, h = 4 * TW + 9, 4 * TH + 1
    img = _img(h, w, 3)
    rank = {"identity": Rank.erode(np.ones((1, 1), np.uint8)), "erode_rect7": Rank.erode(elements.rect(7)),
            "median3": Rank.median(3)}[name]
    got = np.empty_like(img)
    dsrc, ddst = vf_ctx.alloc_device(img.nbytes), vf_ctx.alloc_device(img.nbytes)
    try:
        vf_ctx.upload(dsrc, img, img.nbytes)
        vf_ctx.rank_device(dsrc, ddst, w, h, 3, *rank.args)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, img.nbytes)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    if name == "identity":
        assert np.array_equal(got, img)
    assert np.array_equal(got, R.apply(img, rank.op, 3 if name == "median3" else rank.element))


def test_bands_of_a_frame_larger_than_the_staging():
    """max_frame_bytes = 1 MiB holds 182 rows of a 1080p frame: bands of rows, each uploaded with
    its halo, the border resolved against the frame and not the band."""
    big = np.random.default_rng(9).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    r7 = elements.rect(7)
    frames = [big[:1, :1].copy(), big[:3, :5].copy(), big[:480, :640].copy(), big]
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        want_med = R.median(big, 5)  # once each: the reference is the slow side
        want_ero = R.erode(big, r7, "reflect101")
        assert np.array_equal(vfilter.median_blur(big, 5, ctx=ctx), want_med)
        assert np.array_equal(vfilter.erode(big, r7, border="reflect101", ctx=ctx), want_ero)
        outs = vfilter.rank_frames(frames, Rank.median(5), ctx=ctx)  # a mixed batch: (1,1) (5,3) (640,480) (1920,1080)
        for f, o in zip(frames, outs):
            assert o.shape == f.shape and np.array_equal(o, want_med if f is big else R.median(f, 5)), f.shape
        outs = vfilter.rank_frames(frames, Rank.erode(r7, "reflect101"), ctx=ctx)
        for f, o in zip(frames, outs):
            assert np.array_equal(o, want_ero if f is big else R.erode(f, r7, "reflect101")), f.shape
        # host src is dst, on a frame of three bands: a band's halo rows are the band before's output
        for rank in (Rank.median(5), Rank.dilate(ELEMENTS["random7"], "replicate")):
            buf = big[:400].copy()
            want = R.apply(buf, rank.op, 5 if rank.op == "median" else rank.element, rank.border)
            ctx.rank_frames_host([buf], [buf], [1920], [400], 3, *rank.args)
            assert np.array_equal(buf, want), rank.op


def test_conveniences(vf_ctx):
    img = _img(37, 53, 3)
    c3 = elements.cross(3)
    # element=None is the 3 x 3 rectangle
    assert np.array_equal(vfilter.erode(img, ctx=vf_ctx), R.erode(img, R.rect(3)))
    assert np.array_equal(vfilter.dilate(img, None, ctx=vf_ctx), R.dilate(img, R.rect(3)))
    # an H x W view (non-contiguous) and a plain H x W array
    view = img[:, :, 2]
    assert not view.flags.c_contiguous
    assert np.array_equal(vfilter.median_blur(view, 3, ctx=vf_ctx), R.median(view.copy(), 3))
    flipped = img[::-1, ::2]
    assert np.array_equal(vfilter.dilate(flipped, c3, ctx=vf_ctx), R.dilate(np.ascontiguousarray(flipped), c3))
    gray = img[:, :, 0].copy()
    assert np.array_equal(vfilter.erode(gray, c3, ctx=vf_ctx), R.erode(gray, c3))
    # bools and integers are elements alike
    assert np.array_equal(vfilter.erode(img, c3.astype(bool), ctx=vf_ctx), R.erode(img, c3))
    assert np.array_equal(vfilter.erode(img, c3.astype(np.int64) * 7, ctx=vf_ctx), R.erode(img, c3))
    # dst: filled and returned; refused when it has another shape, dtype or layout
    for fn, want in ((lambda **k: vfilter.erode(img, c3, **k), R.erode(img, c3)),
                     (lambda **k: vfilter.dilate(img, c3, **k), R.dilate(img, c3)),
                     (lambda **k: vfilter.median_blur(img, 5, **k), R.median(img, 5))):
        dst = np.empty_like(img)
        assert fn(dst=dst, ctx=vf_ctx) is dst and np.array_equal(dst, want)
        for bad in (np.empty((37, 53), np.uint8), np.empty(img.shape, np.int8), np.empty((53, 37, 3), np.uint8).transpose(1, 0, 2)):
            with pytest.raises(ValueError):
                fn(dst=bad, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.erode(img, c3, border="wrap", ctx=vf_ctx)
    # erode <= src <= dilate pointwise for an element that holds the centre
    for e in (c3, elements.rect(5, 3), ELEMENTS["rect3x5"]):
        for border in BORDERS:
            lo, hi = vfilter.erode(img, e, border=border, ctx=vf_ctx), vfilter.dilate(img, e, border=border, ctx=vf_ctx)
            assert (lo <= img).all() and (img <= hi).all()
    # an empty frame and an empty batch do nothing
    assert vfilter.erode(np.empty((0, 0, 3), np.uint8), ctx=vf_ctx).shape == (0, 0, 3)
    assert vfilter.rank_frames([], Rank.median(3), ctx=vf_ctx) == []


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _img(9, 11, 3)
    dst = np.empty_like(img)
    probe = Rank.dilate(ELEMENTS["rect3x5"], "reflect101")
    probe_want = R.dilate(img, ELEMENTS["rect3x5"], "reflect101")

    def still_works():
        assert np.array_equal(vfilter.rank_frames([img], probe, ctx=vf_ctx)[0], probe_want)

    ones = np.ones(81, np.uint8)
    zeros = np.zeros(49, np.uint8)
    holed = np.ones(25, np.uint8)
    holed[7] = 0
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)
    E, D, M = 0, 1, 2

    def host(op=E, element=ones, kw=3, kh=3, border=2, channels=3, widths=wa, heights=ha):
        ep = element.ctypes.data if element is not None else None
        return lib.vf_rank_frames_host(vf_ctx.handle, sa, da, widths, heights, 1, channels, op, ep, kw, kh, border)

    refusals = [
        (dict(kw=2), b"element"), (dict(kh=4), b"element"), (dict(kw=9, kh=9), b"element"), (dict(kw=0), b"element"),
        (dict(element=zeros), b"empty element"), (dict(element=zeros, kw=7, kh=7, op=D), b"empty element"),
        (dict(element=None), b"element is NULL"),
        (dict(channels=2), b"channels"), (dict(channels=4), b"channels"),
        (dict(op=3), b"op"), (dict(op=-1), b"op"),
        (dict(border=3), b"border"), (dict(border=-1), b"border"),
        (dict(op=M, border=1, element=holed, kw=5, kh=5), b"median"), (dict(op=M, border=1, kw=3, kh=5), b"median"),
        (dict(op=M, border=1, kw=7, kh=7), b"median"), (dict(op=M, border=1, kw=1, kh=1), b"median"),
        (dict(op=M, border=2), b"median"), (dict(op=M, border=0, kw=5, kh=5), b"median"),
        (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(heights=(ctypes.c_int * 1)(-9)), b"frame"),
    ]
    for kwargs, word in refusals:
        assert host(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        assert word in lib.vf_last_error(vf_ctx.handle)
        still_works()
    assert host() == _lib.VF_OK  # the same call with nothing wrong
    assert host(op=M, border=1, kw=5, kh=5) == _lib.VF_OK
    assert np.array_equal(dst, R.median(img, 5))
    # an empty batch and an empty frame do nothing
    assert lib.vf_rank_frames_host(vf_ctx.handle, None, None, None, None, 0, 3, E, ones.ctypes.data, 3, 3, 2) == _lib.VF_OK
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, op=E, element=ones, kw=3, kh=3, border=2, channels=3, w=11, h=9):
            ep = element.ctypes.data if element is not None else None
            return lib.vf_rank_device(vf_ctx.handle, src, dstp, w, h, channels, op, ep, kw, kh, border, None)

        for kwargs, word in [(dict(kw=2), b"element"), (dict(kw=9), b"element"), (dict(element=zeros), b"empty element"),
                             (dict(element=None), b"element is NULL"), (dict(channels=2), b"channels"),
                             (dict(op=7), b"op"), (dict(border=7), b"border"), (dict(op=M), b"median"),
                             (dict(op=M, border=1, kw=7, kh=7), b"median"), (dict(w=0), b"frame"), (dict(h=-1), b"frame"),
                             (dict(dstp=d), b"overlap"), (dict(dstp=d + n - 1), b"overlap"), (dict(src=d + 1, dstp=d), b"overlap"),
                             (dict(src=None), b"NULL")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK
        assert dev(op=M, border=1) == _lib.VF_OK
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    still_works()


# ---- elements that are not square -----------------------------------------------------------------
# The GPU kernel is compiled for the 3, 5 or 7 square that holds the element: a 1 x 7 element runs as
# 7 x 7 with six rows without members, and stages R = 3 halo rows that a band of vertical radius 0
# does not hold.

OBLONG = R.oblong_set()


def _first_bad_row(got, want):
    """Where two frames differ, by row: for messages."""
    rows = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    return "equal" if rows.size == 0 else "%d rows differ, the first is row %d, the last row %d" % (rows.size, rows[0], rows[-1])


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", list(OBLONG))
@pytest.mark.parametrize("op", ["erode", "dilate"])
def test_oblong_elements_on_straddling_shapes(vf_ctx, op, name, border):
    _sweep(vf_ctx, STRADDLE, op, OBLONG[name], border)


@pytest.mark.parametrize("op,name", [("erode", "1x7"), ("dilate", "7x1")])
@pytest.mark.parametrize("w,c", [(27, 3), (7, 3), (5, 3), (21, 1), (15, 1), (95, 1)])  # W * C mod 16 = 1, 5, 15
@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (1, 5)])
def test_oblong_elements_off_the_16_byte_grid(vf_ctx, op, name, w, c, so, do):
    h = TH + 3
    img = _img(h, w, c)
    n = img.nbytes
    rank = Rank(op, OBLONG[name], "reflect101")
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.rank_device(dsrc + so, ddst + 16 + do, w, h, c, *rank.args)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), R.apply(img, op, OBLONG[name], "reflect101"))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)  # the canaries on both sides


@pytest.mark.parametrize("name", ["1x7", "7x1"])
def test_bands_of_an_oblong_element(name):
    """1024 x 700 x 3 in 1 MiB of staging, which holds 341 rows.  1 x 7 has ry = 0: the bands are rows
    [0, 341), [341, 682), [682, 700) with no halo, and in place nothing is saved, yet the kernel
    (compiled as 7 x 7) stages three rows above and below that the band does not hold.  7 x 1 has
    ry = 3: bands [0, 338), [338, 673), [673, 700), each uploaded from three rows above."""
    big = np.random.default_rng(12).integers(0, 256, (700, 1024, 3), dtype=np.uint8)
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for op, border in (("erode", "reflect101"), ("dilate", "constant")):
            rank = Rank(op, OBLONG[name], border)
            want = R.apply(big, op, OBLONG[name], border)
            got = vfilter.rank_frames([big], rank, ctx=ctx)[0]
            assert np.array_equal(got, want), (name, op, border, _first_bad_row(got, want))
            buf = big.copy()  # host src is dst
            ctx.rank_frames_host([buf], [buf], [1024], [700], 3, *rank.args)
            assert np.array_equal(buf, want), (name, op, border, "in place", _first_bad_row(buf, want))


@pytest.mark.parametrize("w,c", [(1, 3), (3, 1)])
def test_the_row_seam_of_a_launch(vf_ctx, w, c):
    """A launch is split at 65535 x 16 = 1,048,560 rows (the grid's y limit), each part with its own
    first row and destination.  A frame of 1,048,577 rows of 3 bytes crosses the seam: the second
    launch makes rows 1,048,560 to 1,048,576 and its taps reach back over the seam."""
    h = 65535 * TH + 17
    assert h == 1048577
    img = np.random.default_rng([6, w, c]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)
    n = img.nbytes
    for rank in (Rank.erode(ELEMENTS["rect3x5"]), Rank.median(3)):
        want = R.apply(img, rank.op, 3 if rank.op == "median" else rank.element, rank.border)
        got = np.empty_like(img)
        dsrc, ddst = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n)
        try:
            vf_ctx.upload(dsrc, img, n)
            vf_ctx.rank_device(dsrc, ddst, w, h, c, *rank.args)
            vf_ctx.sync()
            vf_ctx.download(got, ddst, n)
            vf_ctx.sync()
        finally:
            vf_ctx.free_device(dsrc)
            vf_ctx.free_device(ddst)
        assert np.array_equal(got, want), (rank.op, "device", _first_bad_row(got, want))
        got = vfilter.rank_frames([img], rank, ctx=vf_ctx)[0]
        assert np.array_equal(got, want), (rank.op, "host", _first_bad_row(got, want))
