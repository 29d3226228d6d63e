"""The resize on raw frames (``vf_resize_*``, ``vfilter.resize``, ``resize_frames``) against the numpy reference of
``tests/_resize_ref.py``.  Every comparison is exact.

Sizes (W x H): 1 x 1 -> 1 x 1 is the smallest frame; 1 x 1 -> 5 x 3 clamps every tap; 5 x 3 -> 1 x 1 shrinks to one
pixel; 9 x 1 and 1 x 9 have one row and one column; 65 x 17 is one pixel wider and one taller than the kernel's
64 x 16 tile, and its double has 3 x 3 tiles; 130 x 34 -> 65 x 17 is where linear runs as area; 67 x 35 -> 100 x 50
and 160 x 48 -> 67 x 35 have scales that are no integers; 300 x 80 -> 75 x 20 has a source box of 256 x 64 pixels a
tile, over the staging budget on three channels and over the h-row budget on both; 300 x 80 -> 20 x 5 is area at
15 x 16.  Every case runs with the kernel's defaults (the box staged, linear per pixel), with the staging switched off
(``VF_RESIZE_LDS=0``), with the h rows switched on (``VF_RESIZE_HROWS=16384``) and with both, against references
computed once and shared.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import _resize_ref as R
import vfilter
from vfilter import Resize, _lib

pytestmark = pytest.mark.gpu

PAIRS = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 3), (1, 1)), ((2, 2), (7, 5)), ((9, 1), (4, 1)), ((1, 9), (1, 20)),
         ((65, 17), (65, 17)), ((65, 17), (130, 34)), ((130, 34), (65, 17)), ((67, 35), (100, 50)), ((160, 48), (67, 35)),
         ((300, 80), (75, 20)), ((300, 80), (20, 5))]
AREA_FACTORS = [(1, 1), (2, 2), (3, 2), (2, 3), (3, 3), (4, 4), (7, 5), (16, 16)]
NAMES = {R.NEAREST: "nearest", R.LINEAR: "linear", R.AREA: "area"}
SWITCHES = ("VF_RESIZE_LDS", "VF_RESIZE_HROWS", "VF_RESIZE_ROWS", "VF_RESIZE_AREA_WIDE")


def _frame(w, h, c):
    return np.random.default_rng([w, h, c, 26]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)


_REF = {}


def _want(w, h, c, dsize, fx, fy, interp):
    """The reference of a case (None where it refuses), computed once and shared by the paths."""
    k = (w, h, c, dsize, fx, fy, interp)
    if k not in _REF:
        try:
            out = R.resize(_frame(w, h, c), dsize, fx, fy, interp)
            out.flags.writeable = False
        except ValueError:
            out = None
        _REF[k] = out
    return _REF[k]


class _Env:
    """The kernel's switches for a block: the library reads them at every launch."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in self.values.items():
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


PATHS = {"defaults": {}, "unstaged": {"VF_RESIZE_LDS": 0}, "h_rows": {"VF_RESIZE_HROWS": 16384},
         "unstaged_h_rows": {"VF_RESIZE_LDS": 0, "VF_RESIZE_HROWS": 16384}}


def _check(ctx, w, h, c, dsize, fx, fy, interp):
    """One case: the bytes, or the refusal where the reference refuses.  True when it ran."""
    img, want = _frame(w, h, c), _want(w, h, c, dsize, fx, fy, interp)
    if want is None:
        with pytest.raises(vfilter.VFilterError, match="integer shrink factors"):
            vfilter.resize(img, dsize, fx, fy, NAMES[interp], ctx=ctx)
        return False
    out = vfilter.resize(img, dsize, fx, fy, NAMES[interp], ctx=ctx)
    assert out.shape == want.shape, (w, h, c, dsize, fx, fy, interp, out.shape, want.shape)
    assert np.array_equal(out, want), (w, h, c, dsize, fx, fy, interp, np.argwhere(out != want)[:5])
    return True


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("c", [1, 3])
def test_every_pair_and_mode(vf_ctx, c, path):
    ran = 0
    with _Env(**PATHS[path]):
        for (w, h), dsize in PAIRS:
            for interp in NAMES:
                ran += _check(vf_ctx, w, h, c, dsize, 0.0, 0.0, interp)
    # area runs for the two identities, 5 x 3 -> 1 x 1, 130 x 34 -> 65 x 17 and 300 x 80 -> 75 x 20 and -> 20 x 5
    assert ran == 2 * len(PAIRS) + 6


def test_what_the_pairs_reach():
    """Without a GPU's help: the modes the pairs resolve to, and the budgets the 300 x 80 shrink is over."""
    assert R.resolve(130, 34, (65, 17), interp=R.LINEAR)[0] == R.AREA
    assert R.resolve(300, 80, (75, 20), interp=R.LINEAR)[0] == R.LINEAR
    assert R.resolve(300, 80, (20, 5), interp=R.AREA)[3:] == (15, 16)
    sx, sy = R.scales(300, 80, (75, 20))
    cs, rs = R.axis_coef(sx, 75, 300, True)[0], R.axis_coef(sy, 20, 80, False)[0]
    box_w, box_h = int(cs[63] + 1 - cs[0] + 1), int(min(rs[15] + 1, 79) - max(rs[0], 0) + 1)  # the first tile's box
    pitch = [(box_w * c + 15) // 16 * 16 for c in (1, 3)]
    assert pitch[0] * box_h <= 16384 < pitch[1] * box_h          # the staged box: inside the budget on 1 channel, over on 3
    assert box_h * 64 * 4 <= 16384 < box_h * 192 * 4             # the h rows likewise


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("dw,dh", [(9, 5), (65, 17)])
def test_area_factor_pairs(vf_ctx, dw, dh, c):
    for k, l in AREA_FACTORS:
        assert _check(vf_ctx, dw * k, dh * l, c, (dw, dh), 0.0, 0.0, R.AREA)
        assert _check(vf_ctx, dw * k, dh * l, c, None, 1.0 / k, 1.0 / l, R.AREA)


@pytest.mark.parametrize("path", ["defaults", "unstaged_h_rows"])
@pytest.mark.parametrize("c", [1, 3])
def test_the_fx_fy_form(vf_ctx, c, path):
    with _Env(**PATHS[path]):
        for (w, h), fx, fy in [((67, 35), 0.3, 0.3), ((5, 5), 0.5, 0.5), ((7, 7), 0.5, 0.5), ((7, 5), 0.5, 0.5), ((67, 35), 0.5, 0.25),
                               ((67, 35), 1.5, 2.25), ((9, 9), 1 / 3, 1 / 3)]:
            ran = [_check(vf_ctx, w, h, c, None, fx, fy, interp) for interp in NAMES]
            assert ran[0] and ran[1]
    assert _want(5, 5, c, None, 0.5, 0.5, R.NEAREST).shape[:2] == (2, 2)  # 2.5 rounds to even
    assert _want(7, 7, c, None, 0.5, 0.5, R.NEAREST).shape[:2] == (4, 4)  # and 3.5 as well
    assert _want(67, 35, c, None, 0.3, 0.3, R.LINEAR).shape[:2] == (10, 20)  # 10.5 and 20.1
    assert _want(7, 7, c, None, 0.5, 0.5, R.AREA) is not None  # the last block overruns the frame: cv2's slow tail


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("c", [1, 3])
def test_area_two_by_two_with_wide_loads_and_without(vf_ctx, c, wide):
    """The wide-load kernel runs where the source's rows are a multiple of 4 bytes (W % 4 == 0 on both channel
    counts): 132 -> 66 ends a row's second tile with a lane of 2 valid bytes on both channel counts, and a result row
    of 66 or 198 bytes makes every other row's dword stores unaligned; 35 rows at fy = 0.5 make 18, whose last block
    row overruns the frame; 256 x 64 is whole tiles only; 130 -> 65 has rows of 130 and 390 bytes, so it stays with the
    byte kernel whatever the switch says.  The references are shared, so both kernels give the same bytes."""
    with _Env(VF_RESIZE_AREA_WIDE=wide):
        for (w, h), dsize, fx, fy in [((132, 34), (66, 17), 0.0, 0.0), ((132, 35), None, 0.5, 0.5), ((256, 64), (128, 32), 0.0, 0.0),
                                      ((4, 2), (2, 1), 0.0, 0.0), ((130, 34), (65, 17), 0.0, 0.0), ((264, 70), None, 0.5, 0.5)]:
            for interp in (R.LINEAR, R.AREA):  # linear at 2 x 2 runs as area
                assert _check(vf_ctx, w, h, c, dsize, fx, fy, interp)
        for rows in (1, 5, 64):
            with _Env(VF_RESIZE_AREA_WIDE=wide, VF_RESIZE_ROWS=rows):
                assert _check(vf_ctx, 132, 35, c, None, 0.5, 0.5, R.AREA)


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("c", [1, 3])
def test_area_at_other_factors_with_wide_loads_and_without(vf_ctx, c, wide):
    """The wide-load kernel of the factors other than 2 x 2 runs where W % 4 == 0.  Block rows of 1 to 48 bytes that
    start at every residue of 4 and, on 3 channels, at every channel phase: factors 1, 3, 4, 5, 7, 15 and 16 across
    a row of 65 or more pixels; 68 pixels make a second tile of 4; 24 x 11 at fx = 1 / 3, fy = 0.5 makes 6 rows
    whose last block row overruns the frame; 195 -> 65 has rows of 195 and 585 bytes and stays with the byte kernel."""
    with _Env(VF_RESIZE_AREA_WIDE=wide):
        for (k, l), (dw, dh) in [((1, 1), (68, 5)), ((3, 2), (68, 9)), ((4, 4), (65, 17)), ((5, 3), (68, 4)), ((7, 5), (68, 3)),
                                 ((15, 16), (20, 5)), ((16, 16), (65, 3)), ((16, 1), (8, 7)), ((1, 16), (8, 3)), ((3, 3), (65, 5))]:
            assert _check(vf_ctx, dw * k, dh * l, c, (dw, dh), 0.0, 0.0, R.AREA)
        assert _check(vf_ctx, 24, 11, c, None, 1 / 3, 0.5, R.AREA)
        assert _want(24, 11, c, None, 1 / 3, 0.5, R.AREA).shape[:2] == (6, 8)
        for rows in (1, 5, 64):
            with _Env(VF_RESIZE_AREA_WIDE=wide, VF_RESIZE_ROWS=rows):
                assert _check(vf_ctx, 272, 51, c, (68, 17), 0.0, 0.0, R.AREA)


MAX_ROWS, MAX_LDS = 64, 30720  # csrc/vf_resize.hip kMaxTileRows, kMaxLds
# (VF_RESIZE_ROWS, VF_RESIZE_LDS, VF_RESIZE_HROWS): 100 rows clamp to 64 and 0 to 1; 1000 bytes round down to 992 and
# 1000000 clamp to the cap; 16 bytes stage a box of one row of at most 16 bytes and hold no h row
EXTREMES = [(1, 16, 16), (1, MAX_LDS, MAX_LDS), (5, 1000, 0), (5, 0, 1000), (16, MAX_LDS, 0), (16, 0, MAX_LDS), (64, 1000, 1000),
            (64, MAX_LDS, MAX_LDS), (64, 1000000, 1000000), (100, 16, 1000000), (100, 1000000, 16), (0, 1000, MAX_LDS), (0, 0, 0)]


@pytest.mark.parametrize("c", [1, 3])
def test_the_switches_change_no_byte(vf_ctx, c):
    for rows, lds, hlds in EXTREMES:
        with _Env(VF_RESIZE_ROWS=rows, VF_RESIZE_LDS=lds, VF_RESIZE_HROWS=hlds):
            for (w, h), dsize in [((67, 35), (100, 50)), ((160, 48), (67, 35)), ((70, 130), (35, 65)), ((70, 130), (23, 26))]:
                for interp in NAMES:
                    _check(vf_ctx, w, h, c, dsize, 0.0, 0.0, interp)


def test_frames_of_mixed_sizes_in_one_call(vf_ctx):
    frames = [_frame(67, 35, 3), _frame(5, 7, 3), np.zeros((0, 0, 3), np.uint8), _frame(160, 48, 3)]
    f = Resize(fx=0.3, fy=0.75, interpolation="linear")
    outs = vfilter.resize_frames(frames, f, ctx=vf_ctx)
    assert outs[2].shape == (0, 0, 3)
    for img, out in zip(frames, outs):
        if img.size:
            assert np.array_equal(out, R.resize(img, None, 0.3, 0.75, R.LINEAR))
            assert out.shape[:2] == f.out_size(img.shape[1], img.shape[0])[::-1]
            assert vf_ctx.resize_out_size(img.shape[1], img.shape[0], *f.args) == f.out_size(img.shape[1], img.shape[0])
    given = [np.empty_like(o) for o in outs]
    assert vfilter.resize_frames(frames, f, given, ctx=vf_ctx) is not None and all(np.array_equal(a, b) for a, b in zip(given, outs))
    gray = vfilter.resize_frames([_frame(9, 9, 1)], Resize((4, 3), interpolation=0), ctx=vf_ctx)[0]
    assert gray.shape == (3, 4) and np.array_equal(gray, R.resize(_frame(9, 9, 1), (4, 3), interp=R.NEAREST))


def test_the_last_bytes_of_the_frame_are_staged_without_reading_past_them(vf_ctx):
    """Device allocations that end with their frames: the last tile's box ends at the source's last byte, where a
    16-byte load would cross the end."""
    for (w, h, c), dsize, interp in [((67, 35, 3), (67, 35), R.LINEAR), ((65, 17, 1), (130, 34), R.LINEAR), ((5, 7, 3), (9, 11), R.NEAREST),
                                     ((66, 34, 3), (33, 17), R.AREA)]:
        img = _frame(w, h, c)
        want = R.resize(img, dsize, interp=interp)
        got = np.empty(want.shape, np.uint8)
        dsrc, ddst = vf_ctx.alloc_device(img.nbytes), vf_ctx.alloc_device(want.nbytes)
        try:
            vf_ctx.upload(dsrc, img, img.nbytes)
            vf_ctx.resize_device(dsrc, ddst, w, h, c, dsize[0], dsize[1], 0.0, 0.0, interp)
            vf_ctx.sync()
            vf_ctx.download(got, ddst, want.nbytes)
            vf_ctx.sync()
        finally:
            for p in (dsrc, ddst):
                vf_ctx.free_device(p)
        assert np.array_equal(got, want), (w, h, c, dsize, interp)


def test_the_filter_value():
    f = Resize((4, 3))
    assert f.args == (4, 3, 0.0, 0.0, 1) and f.interpolation == "linear" and f.out_size(100, 50) == (4, 3)
    assert Resize(None, 0.5, 0.5, 3).interpolation == "area" and Resize((0, 0), 2, 2, "nearest").args == (0, 0, 2.0, 2.0, 0)
    assert Resize(fx=0.5, fy=0.5).out_size(5, 7) == (2, 4)
    with pytest.raises(dataclasses.FrozenInstanceError):
        f.fx = 1.0
    for bad, word in [(dict(interpolation=2), "not built"), (dict(interpolation=4), "not built"), (dict(interpolation="cubic"), "one of"),
                      (dict(interpolation=5), "one of"), (dict(interpolation=True), "one of"), (dict(dsize=(4,)), "dsize is"),
                      (dict(dsize=(4.5, 3)), "dsize is"), (dict(dsize=(0, 3)), "a side is 1 to 32767"),
                      (dict(dsize=(32768, 3)), "a side is 1 to 32767"), (dict(), "finite and positive"),
                      (dict(fx=0.5), "finite and positive"), (dict(fx=-1, fy=1), "finite and positive"),
                      (dict(fx=float("nan"), fy=1), "finite and positive"), (dict(fx="a", fy=1), "are numbers")]:
        with pytest.raises(ValueError, match=word):
            Resize(**bad)
    with pytest.raises(ValueError, match="a side of 0"):
        Resize(fx=0.1, fy=0.1).out_size(3, 3)
    with pytest.raises(ValueError, match="a side is at most 32767"):
        Resize(fx=2, fy=1).out_size(30000, 3)


def test_refusals_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _frame(12, 12, 3)
    probe_want = R.resize(img, (7, 5))

    def still_works():
        assert np.array_equal(vfilter.resize(img, (7, 5), ctx=vf_ctx), probe_want)

    for call, word in [(lambda: vfilter.resize(img, (8, 8), interpolation="area", ctx=vf_ctx), "integer shrink factors"),  # 1.5 x
                       (lambda: vfilter.resize(img, (24, 12), interpolation="area", ctx=vf_ctx), "integer shrink factors"),
                       (lambda: vfilter.resize(img, (7, 5), dst=np.empty((5, 8, 3), np.uint8), ctx=vf_ctx), "result's shape"),
                       (lambda: vfilter.resize(img, (7, 5), dst=np.empty((7, 5, 3), np.uint8), ctx=vf_ctx), "result's shape"),
                       (lambda: vfilter.resize(img, fx=0.01, fy=0.01, ctx=vf_ctx), "a side of 0"),
                       (lambda: vfilter.resize(img, (32768, 5), ctx=vf_ctx), "a side is 1 to 32767")]:
        with pytest.raises((ValueError, vfilter.VFilterError), match=word):
            call()
        still_works()

    dst = np.empty((5, 7, 3), np.uint8)
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(12), (ctypes.c_int * 1)(12)
    D = ctypes.c_double

    def host(dw=7, dh=5, fx=0.0, fy=0.0, interp=1, channels=3, srcs=sa, dsts=da, widths=wa, heights=ha, n=1):
        return lib.vf_resize_frames_host(vf_ctx.handle, srcs, dsts, widths, heights, n, channels, dw, dh, D(fx), D(fy), interp)

    nan, inf = float("nan"), float("inf")
    for kwargs, word in [(dict(interp=2), b"is not built"), (dict(interp=4), b"is not built"), (dict(interp=5), b"unknown interpolation 5"),
                         (dict(interp=-1), b"unknown interpolation -1"), (dict(dw=32768), b"a side is 1 to 32767"),
                         (dict(dw=-1), b"a side is 1 to 32767"), (dict(dw=0), b"has a side of 0"), (dict(dh=0), b"has a side of 0"),
                         (dict(dw=0, dh=0), b"finite and positive"), (dict(dw=0, dh=0, fx=0.5), b"finite and positive"),
                         (dict(dw=0, dh=0, fx=nan, fy=1), b"finite and positive"), (dict(dw=0, dh=0, fx=inf, fy=1), b"finite and positive"),
                         (dict(dw=0, dh=0, fx=0.01, fy=0.01), b"frame 0: step 1: a frame of 12 x 12 resizes to 0 x 0: a side of 0"),
                         (dict(dw=0, dh=0, fx=5000, fy=1), b"resizes to 60000 x 12; a side is at most 32767"),
                         (dict(dw=8, dh=8, interp=3), b"frame 0: step 1: area from 12 x 12 to 8 x 8"),
                         (dict(channels=2), b"channels=2"),
                         (dict(widths=(ctypes.c_int * 1)(32768), heights=(ctypes.c_int * 1)(1)), b"a side is at most 32767"),
                         (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(srcs=(ctypes.c_void_p * 1)(None)), b"NULL buffer"),
                         (dict(n=-1), b"n < 0"),
                         (dict(dsts=sa), b"overlap"), (dict(dsts=(ctypes.c_void_p * 1)(img.ctypes.data + img.nbytes - 1)), b"overlap")]:
        assert host(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(vf_ctx.handle), (kwargs, lib.vf_last_error(vf_ctx.handle))
        still_works()
    assert host() == _lib.VF_OK and np.array_equal(dst, probe_want)
    same = img.copy()  # equal sizes: in place is allowed, the source is the staged copy
    assert host(dw=12, dh=12, srcs=(ctypes.c_void_p * 1)(same.ctypes.data), dsts=(ctypes.c_void_p * 1)(same.ctypes.data)) == _lib.VF_OK
    assert np.array_equal(same, img)
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, w=12, h=12, channels=3, dw=7, dh=5, fx=0.0, fy=0.0, interp=1):
            return lib.vf_resize_device(vf_ctx.handle, src, dstp, w, h, channels, dw, dh, D(fx), D(fy), interp, None)

        for kwargs, word in [(dict(dstp=d), b"src and dst overlap"), (dict(dstp=d + n - 1), b"src and dst overlap"),
                             (dict(src=d + 7 * 5 * 3 - 1, dstp=d), b"src and dst overlap"),
                             (dict(dw=12, dh=12, dstp=d), b"src and dst overlap"),  # not even at equal sizes
                             (dict(src=None), b"NULL buffer"), (dict(dstp=None), b"NULL buffer"), (dict(interp=2), b"is not built"),
                             (dict(dw=8, dh=8, interp=3), b"area from 12 x 12 to 8 x 8"), (dict(dw=32768), b"a side is 1 to 32767"),
                             (dict(w=32768, h=1, channels=1), b"a side is at most 32767"), (dict(w=0), b"frame"),
                             (dict(dw=0, dh=0, fx=0.01, fy=0.01), b"a side of 0"), (dict(channels=2), b"channels=2")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(vf_ctx.handle), (kwargs, lib.vf_last_error(vf_ctx.handle))
            still_works()
        assert dev() == _lib.VF_OK
        assert dev(src=d + 7 * 5 * 3, dstp=d) == _lib.VF_OK  # the result ends where the source starts
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)

    ow, oh = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vf_resize_out_size(vf_ctx.handle, 12, 12, 0, 0, D(0.01), D(0.01), 1, ctypes.byref(ow), ctypes.byref(oh)) == _lib.VF_E_INVALID
    assert b"a side of 0" in lib.vf_last_error(vf_ctx.handle)
    assert lib.vf_resize_out_size(vf_ctx.handle, 5, 7, 0, 0, D(0.5), D(0.5), 1, ctypes.byref(ow), ctypes.byref(oh)) == _lib.VF_OK
    assert (ow.value, oh.value) == (2, 4)


def test_a_frame_or_a_result_larger_than_the_staging():
    big = np.random.default_rng(12).integers(0, 256, (600, 700, 3), dtype=np.uint8)
    small = np.ascontiguousarray(big[:100])
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        with pytest.raises(vfilter.VFilterError, match="value 0 of 700 x 600 .* does not fit the context's"):
            vfilter.resize(big, (70, 60), ctx=ctx)
        with pytest.raises(vfilter.VFilterError, match="value 1 of 1400 x 600 .* does not fit the context's"):
            vfilter.resize(small, (1400, 600), interpolation="nearest", ctx=ctx)
        assert np.array_equal(vfilter.resize(small, (70, 10), ctx=ctx), R.resize(small, (70, 10)))
