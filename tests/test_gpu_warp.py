"""The affine warp on raw frames (``vf_warp_*``, ``vfilter.warp_affine``, ``flip``, ``rotate``, ``warp_frames``) against
the numpy reference of ``tests/_warp_ref.py``.  Every comparison is exact.

Sizes (W x H): 1 x 1, 1 x 9, 9 x 1 and 2 x 2 have axes on which a saturated coordinate reflects thousands of times;
5 x 7; 65 x 17 is one pixel wider and one taller than the kernel's 64 x 16 tile; 67 x 35 and 160 x 48 have several
tiles on both axes, so a rotation about the centre gives tiles whose source box is inside the frame (staged in LDS)
and tiles that touch the border (gathered from global memory) in one frame.  300 x 80 under the 0.25 x shrink has a
box inside the frame that is over the LDS budget on three channels.  Every case runs again with ``VF_WARP_LDS=0``,
which forces the general path everywhere; the references are computed once and shared.  70 x 130 and the map
``rows_x2`` are there for ``test_the_tile_switches_change_no_byte``, which sets ``VF_WARP_ROWS`` and ``VF_WARP_LDS``
(``tests/test_warp_tile_switches.py`` holds, without a GPU, what those cases reach).
"""
import ctypes
import os

import numpy as np
import pytest

import _warp_ref as R
import vfilter
from vfilter import Warp, _lib, warps

pytestmark = pytest.mark.gpu

TILE_W, TILE_H, LDS = 64, 16, 16384  # csrc/vf_warp.hip kTileW, kTileRows, kWarpLds
SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (TILE_W + 1, TILE_H + 1), (67, 35), (160, 48)]  # (W, H)
BORDER_NAMES = {R.REFLECT101: "reflect101", R.REPLICATE: "replicate", R.CONSTANT: "constant"}
VALUE = (201, 7, 99)


def _frame(w, h, c):
    return np.random.default_rng([w, h, c]).integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)


def _maps(w, h):
    """name -> (mode, m): m maps destination to source."""
    centre = ((w - 1) / 2, (h - 1) / 2)
    return {
        "identity": (0, [1, 0, 0, 0, 1, 0]),
        "flip_h": (1, None), "flip_v": (2, None), "flip_both": (3, None),
        "shift_whole": (0, [1, 0, -3, 0, 1, 2]),
        "shift_half": (0, [1, 0, 0.5, 0, 1, 0.5]),
        "shift_32nds": (0, [1, 0, 5 / 32, 0, 1, -11 / 32]),
        "rotate30_scale1.3": (0, R.invert_affine(R.rotation(centre, 30.0, 1.3))),
        "shrink_0.25": (0, [4, 0, 0, 0, 4, 0]),
        "saturating": (0, [1, 0, 999999, 0, 1, -999998]),
        "negative_determinant": (0, [0.6, 0.8, -3.5, 0.8, -0.6, 2.5]),
        # two source rows an output row: a tile of 64 rows reads a box of 128, more than the default LDS budget holds
        "rows_x2": (0, [1, 0, 0.25, 0, 2, 0.5]),
    }


def _filter(mode, m, interp, border):
    name = "linear" if interp == R.LINEAR else "nearest"
    if mode:
        f = Warp(flip={1: "h", 2: "v", 3: "both"}[mode], interpolation=name, border=BORDER_NAMES[border], border_value=VALUE)
    else:
        f = Warp(np.array(m, np.float64).reshape(2, 3), None, name, BORDER_NAMES[border], VALUE, inverse_map=True)
    assert f.args == (None if mode else tuple(float(v) for v in m), mode, interp, border, VALUE)
    return f


_REF = {}


def _want(w, h, c, name, interp, border):
    """The reference of a case, computed once and shared by the two paths."""
    k = (w, h, c, name, interp, border)
    if k not in _REF:
        mode, m = _maps(w, h)[name]
        out = R.warp(_frame(w, h, c), m, mode, interp, border, VALUE)
        out.flags.writeable = False
        _REF[k] = out
    return _REF[k]


@pytest.fixture
def general_path():
    """``VF_WARP_LDS=0`` for the test: the library reads the switch at every launch."""
    old = os.environ.get("VF_WARP_LDS")
    os.environ["VF_WARP_LDS"] = "0"
    yield
    if old is None:
        del os.environ["VF_WARP_LDS"]
    else:
        os.environ["VF_WARP_LDS"] = old


def _every_case(ctx, c, interp):
    for w, h in SIZES + [(300, 80)]:
        img = _frame(w, h, c)
        for name, (mode, m) in _maps(w, h).items():
            if (w, h) == (300, 80) and name not in ("shrink_0.25", "rotate30_scale1.3"):
                continue
            for border in BORDER_NAMES:
                out = vfilter.warp_frames([img], _filter(mode, m, interp, border), ctx=ctx)[0]
                want = _want(w, h, c, name, interp, border)
                assert out.shape == img.shape and np.array_equal(out, want), (w, h, name, border, np.argwhere(out != want)[:5])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
def test_every_size_map_and_border(vf_ctx, interp, c):
    _every_case(vf_ctx, c, interp)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
def test_every_size_map_and_border_on_the_general_path(vf_ctx, general_path, interp, c):
    """The same cases against the same references, so both paths give the same bytes."""
    _every_case(vf_ctx, c, interp)


MAX_ROWS, MAX_LDS = 64, 61440  # csrc/vf_warp.hip kMaxTileRows, kMaxWarpLds
# (VF_WARP_ROWS, VF_WARP_LDS): 100 rows clamp to 64 and 0 to 1; 1000 bytes round down to 992 and 1000000 clamp to the
# cap; 16 bytes hold a box of one row of at most 16 bytes, so nearly every tile takes the general path.  64 rows
# meet both large budgets, where the dynamic LDS and the row bases together come close to 64 KiB.
SWITCHES = [(1, 16), (1, 61440), (5, 16), (5, 1000), (16, 61440), (64, 1000), (64, 61440), (64, 1000000), (100, 16),
            (100, 1000000), (0, 1000), (0, 61440)]
SWITCH_SIZES = [(TILE_W + 1, TILE_H + 1), (67, 35), (160, 48), (70, 130)]  # 70 x 130: a full tile of 64 rows, and a third row of tiles
SWITCH_MAPS = ["rotate30_scale1.3", "shrink_0.25", "shift_32nds", "flip_both", "rows_x2"]


def _clamped(rows, lds):
    """What ``launch_warp`` makes of the two switches."""
    return min(max(rows, 1), MAX_ROWS), min(lds, MAX_LDS) // 16 * 16


@pytest.fixture
def tile_switches():
    """A setter of ``VF_WARP_ROWS`` and ``VF_WARP_LDS``, which the library reads at every launch; both are put back."""
    old = {k: os.environ.get(k) for k in ("VF_WARP_ROWS", "VF_WARP_LDS")}

    def set_both(rows, lds):
        os.environ["VF_WARP_ROWS"], os.environ["VF_WARP_LDS"] = str(rows), str(lds)

    yield set_both
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("interp", [R.LINEAR, R.NEAREST])
def test_the_tile_switches_change_no_byte(vf_ctx, tile_switches, interp, c):
    """A tile of 1 to 64 rows under a budget of 16 bytes to the cap, against the same references: a switch may
    change the path a tile takes, never a byte."""
    for rows, lds in SWITCHES:
        tile_switches(rows, lds)
        for w, h in SWITCH_SIZES + [(300, 80)]:
            img = _frame(w, h, c)
            for name in SWITCH_MAPS if (w, h) != (300, 80) else ["shrink_0.25"]:
                mode, m = _maps(w, h)[name]
                for border in BORDER_NAMES:
                    out = vfilter.warp_frames([img], _filter(mode, m, interp, border), ctx=vf_ctx)[0]
                    want = _want(w, h, c, name, interp, border)
                    assert out.shape == img.shape and np.array_equal(out, want), \
                        (rows, lds, w, h, name, border, np.argwhere(out != want)[:5])


def _tile_boxes(w, h, c, m, interp, rows=TILE_H, budget=LDS):
    """Per tile of the output, a tile ``rows`` rows under a budget of ``budget`` bytes: ("lds", "border" (the box
    leaves the frame) or "budget", the bytes of its box in LDS), from the reference's coordinates."""
    sx, sy, _, _ = R.coords(m, w, h, interp)
    second = 1 if interp == R.LINEAR else 0
    out = []
    for y0 in range(0, h, rows):
        for x0 in range(0, w, TILE_W):
            bx, by = sx[y0:y0 + rows, x0:x0 + TILE_W], sy[y0:y0 + rows, x0:x0 + TILE_W]
            lo_x, hi_x, lo_y, hi_y = bx.min(), bx.max() + second, by.min(), by.max() + second
            if lo_x < 0 or hi_x >= w or lo_y < 0 or hi_y >= h:
                out.append(("border", 0))
            else:
                pitch = ((hi_x - lo_x + 1) * c + 15) // 16 * 16
                size = int(pitch * (hi_y - lo_y + 1))
                out.append(("lds" if size <= budget else "budget", size))
    return out


def _tile_paths(w, h, c, m, interp, rows=TILE_H, budget=LDS):
    return [path for path, _ in _tile_boxes(w, h, c, m, interp, rows, budget)]


def test_the_frames_are_what_they_are_chosen_for():
    """Needs no GPU, but belongs to the cases above: the rotation has interior and border tiles in one frame, the
    shrink a box that is over the budget, and the two interpolations give different pictures."""
    for w, h in [(67, 35), (160, 48)]:
        paths = _tile_paths(w, h, 3, _maps(w, h)["rotate30_scale1.3"][1], R.LINEAR)
        assert "lds" in paths and "border" in paths, (w, h, paths)
    assert _tile_paths(300, 80, 3, [4, 0, 0, 0, 4, 0], R.LINEAR)[0] == "budget"
    assert _tile_paths(300, 80, 1, [4, 0, 0, 0, 4, 0], R.LINEAR)[0] == "lds"
    assert set(_tile_paths(TILE_W + 1, TILE_H + 1, 3, [1, 0, 0, 0, 1, 0], R.NEAREST)) == {"lds"} and \
        len(_tile_paths(TILE_W + 1, TILE_H + 1, 3, [1, 0, 0, 0, 1, 0], R.NEAREST)) == 4
    a = _want(160, 48, 3, "rotate30_scale1.3", R.LINEAR, R.CONSTANT)
    b = _want(160, 48, 3, "rotate30_scale1.3", R.NEAREST, R.CONSTANT)
    c = _want(160, 48, 3, "rotate30_scale1.3", R.LINEAR, R.REPLICATE)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.any(np.all(a == np.array(VALUE, np.uint8), axis=2))  # the border colour shows, every channel its own


def test_the_drop_ins(vf_ctx):
    img = _frame(67, 35, 3)
    gray = _frame(160, 48, 1)
    assert np.array_equal(vfilter.flip(img, 1, ctx=vf_ctx), img[:, ::-1])
    assert np.array_equal(vfilter.flip(img, 0, ctx=vf_ctx), img[::-1])
    assert np.array_equal(vfilter.flip(gray, -1, ctx=vf_ctx), gray[::-1, ::-1])
    assert np.array_equal(vfilter.flip(gray, 5, ctx=vf_ctx), gray[:, ::-1])  # cv2: any positive code
    assert np.array_equal(vfilter.rotate(img, "180", ctx=vf_ctx), img[::-1, ::-1])
    assert np.array_equal(vfilter.rotate(img, 1, ctx=vf_ctx), img[::-1, ::-1])  # cv2.ROTATE_180
    fwd = warps.rotation((33, 17), 30.0, 1.3)
    m = R.invert_affine(fwd)
    assert np.array_equal(vfilter.warp_affine(img, fwd, ctx=vf_ctx), R.warp(img, m))
    assert np.array_equal(vfilter.warp_affine(img, fwd, (67, 35), flags=vfilter.filters.INTER_NEAREST, ctx=vf_ctx),
                          R.warp(img, m, interp=R.NEAREST))
    inv = np.array(m).reshape(2, 3)
    assert np.array_equal(vfilter.warp_affine(img, inv, flags=vfilter.filters.INTER_LINEAR | vfilter.filters.WARP_INVERSE_MAP,
                                              border="replicate", ctx=vf_ctx), R.warp(img, m, border=R.REPLICATE))
    assert np.array_equal(vfilter.warp_affine(img, warps.translation(2.5, -1.25), border="reflect101", ctx=vf_ctx),
                          R.warp(img, [1, 0, -2.5, 0, 1, 1.25], border=R.REFLECT101))
    assert np.array_equal(vfilter.warp_affine(gray, warps.zoom(2.0, (80, 24)), border_value=50, ctx=vf_ctx),
                          R.warp(gray, [0.5, 0, 40, 0, 0.5, 12], value=50))
    view = img[:, :, 1]  # not contiguous
    assert np.array_equal(vfilter.flip(view, 1, ctx=vf_ctx), view[:, ::-1])
    buf = img.copy()  # the host path takes src == dst: its source is the staged copy
    assert vfilter.flip(buf, -1, dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, img[::-1, ::-1])
    buf = img.copy()
    assert vfilter.warp_affine(buf, fwd, dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, R.warp(img, m))
    with pytest.raises(ValueError, match="frames keep their size"):
        vfilter.warp_affine(img, fwd, (35, 67), ctx=vf_ctx)
    for code in ("90_clockwise", "90_counterclockwise", 0, 2):
        with pytest.raises(ValueError, match="frames keep their size"):
            vfilter.rotate(img, code, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.warp_affine(img.astype(np.int16), fwd, ctx=vf_ctx)


def test_warp_frames_with_mixed_sizes_under_one_flip(vf_ctx):
    for c in (1, 3):
        frames = [_frame(5, 7, c), np.empty((0, 0, 3) if c == 3 else (0, 0), np.uint8), _frame(160, 48, c), _frame(1, 9, c),
                  _frame(67, 35, c)]
        for f, view in ((Warp(flip="h"), lambda a: a[:, ::-1]), (Warp(flip="v"), lambda a: a[::-1]),
                        (Warp(flip="both", interpolation="nearest"), lambda a: a[::-1, ::-1])):
            outs = vfilter.warp_frames(frames, f, ctx=vf_ctx)
            assert len(outs) == len(frames)
            for a, o in zip(frames, outs):
                assert o.shape == a.shape and np.array_equal(o, view(a)), (a.shape, f.mode)
        f = Warp(warps.translation(1.5, 0.25), border="replicate")
        filled = [np.empty_like(a) for a in frames]
        assert vfilter.warp_frames(frames, f, outs=filled, ctx=vf_ctx) is filled
        for a, o in zip(frames, filled):
            assert np.array_equal(o, R.warp(a, f.m, border=R.REPLICATE))
    assert vfilter.warp_frames([], Warp(flip="h"), ctx=vf_ctx) == []


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("so,do", [(0, 0), (1, 1), (7, 7), (15, 15), (3, 8), (0, 5), (9, 0), (15, 1)])
def test_device_buffers_off_the_16_byte_grid(vf_ctx, c, so, do):
    """The staging's 16-byte loads take any alignment and read nothing past the frame; canaries on both sides."""
    w, h = 160, 48
    img = _frame(w, h, c)
    n = img.nbytes
    m = _maps(w, h)["rotate30_scale1.3"][1]
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.warp_device(dsrc + so, ddst + 16 + do, w, h, c, m, 0, R.LINEAR, R.CONSTANT, VALUE)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        for p in (dsrc, ddst):
            vf_ctx.free_device(p)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), _want(w, h, c, "rotate30_scale1.3", R.LINEAR, R.CONSTANT))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)


def test_the_last_bytes_of_the_frame_are_staged_without_reading_past_them(vf_ctx):
    """An identity over a frame whose device allocation ends with the frame: the last tile's box ends at the frame's
    last byte, where a 16-byte load would cross the end."""
    for w, h, c in [(67, 35, 3), (65, 17, 1), (5, 7, 3)]:
        img = _frame(w, h, c)
        n = img.nbytes
        got = np.empty_like(img)
        dsrc, ddst = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n)
        try:
            vf_ctx.upload(dsrc, img, n)
            vf_ctx.warp_device(dsrc, ddst, w, h, c, [1, 0, 0, 0, 1, 0], 0, R.LINEAR, R.REFLECT101, (0, 0, 0))
            vf_ctx.sync()
            vf_ctx.download(got, ddst, n)
            vf_ctx.sync()
        finally:
            for p in (dsrc, ddst):
                vf_ctx.free_device(p)
        assert np.array_equal(got, img), (w, h, c)


def test_a_frame_larger_than_the_staging():
    big = np.random.default_rng(12).integers(0, 256, (600, 700, 3), dtype=np.uint8)
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for call in (lambda: vfilter.flip(big, 1, ctx=ctx),
                     lambda: vfilter.chain(big, [Warp(flip="v"), vfilter.filters.Invert()], ctx=ctx)):
            with pytest.raises(vfilter.VFilterError) as e:
                call()
            assert "600 rows of 2100 bytes do not fit the context's" in str(e.value) and "staging" in str(e.value)
        small = np.ascontiguousarray(big[:100])  # and the context still works, on a frame that fits
        assert np.array_equal(vfilter.flip(small, 1, ctx=ctx), small[:, ::-1])


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _frame(11, 9, 3)
    dst = np.empty_like(img)
    ident = (ctypes.c_double * 6)(1, 0, 0.5, 0, 1, 0.25)
    probe_want = R.warp(img, list(ident))
    zero = (ctypes.c_int * 3)(0, 0, 0)

    def still_works():
        assert np.array_equal(vfilter.warp_affine(img, np.array(list(ident)).reshape(2, 3), inverse_map=True, ctx=vf_ctx), probe_want)

    def dmap(*vals):
        return (ctypes.c_double * 6)(*vals)

    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)

    def host(m=ident, mode=0, interp=0, border=2, value=zero, channels=3, srcs=sa, dsts=da, widths=wa, heights=ha, n=1):
        return lib.vf_warp_frames_host(vf_ctx.handle, srcs, dsts, widths, heights, n, channels, m, mode, interp, border, value)

    null1 = (ctypes.c_void_p * 1)(None)
    inf, nan = float("inf"), float("nan")
    refusals = [
        (dict(mode=4), b"mode=4 outside 0..3"), (dict(mode=-1), b"mode=-1"), (dict(interp=2), b"interp=2 outside 0..1"),
        (dict(border=3), b"unknown border 3"), (dict(border=-1), b"unknown border -1"),
        (dict(value=(ctypes.c_int * 3)(0, 256, 0)), b"value[1]=256 outside 0..255"),
        (dict(value=(ctypes.c_int * 3)(-1, 0, 0)), b"value[0]=-1"), (dict(value=None), b"value is NULL"),
        (dict(m=None), b"m is NULL"), (dict(m=dmap(1, 0, inf, 0, 1, 0)), b"m[2] is not finite"),
        (dict(m=dmap(nan, 0, 0, 0, 1, 0)), b"m[0] is not finite"), (dict(m=dmap(1, 0, 0, 0, -inf, 0)), b"m[4] is not finite"),
        (dict(m=dmap(1e6, 0, 0, 0, 1, 0)), b"frame 0: m[0]="), (dict(m=dmap(1, 0, 0, -1e6, 1, 0)), b"frame 0: m[3]="),
        (dict(m=dmap(1, 0, 1048576, 0, 1, 0)), b"frame 0: m[1]=0.000000 and m[2]=1048576"),
        (dict(m=dmap(1, 0, 0, 0, 1, -2e6)), b"frame 0: m[4]=1.000000 and m[5]=-2000000"),
        (dict(m=dmap(1, 2e5, 0, 0, 1, 0)), b"at row 8"),
        (dict(channels=2), b"channels=2"), (dict(channels=4), b"channels=4"),
        (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(heights=(ctypes.c_int * 1)(-9)), b"frame"),
        (dict(widths=(ctypes.c_int * 1)(32768), heights=(ctypes.c_int * 1)(1)), b"a side is at most 32767"),
        (dict(widths=(ctypes.c_int * 1)(1), heights=(ctypes.c_int * 1)(32768)), b"a side is at most 32767"),
        (dict(srcs=null1), b"NULL buffer"), (dict(dsts=null1), b"NULL buffer"), (dict(srcs=None), b"NULL array"),
        (dict(n=-1), b"n < 0"),
        (dict(dsts=(ctypes.c_void_p * 1)(img.ctypes.data + 3)), b"partially overlap"),
    ]
    for kwargs, word in refusals:
        assert host(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        assert word in lib.vf_last_error(vf_ctx.handle)
        still_works()
    assert host() == _lib.VF_OK and np.array_equal(dst, probe_want)
    assert host(mode=1, m=None) == _lib.VF_OK and np.array_equal(dst, img[:, ::-1])  # a flip reads no m
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK
    assert host(m=dmap(1, 0, 999999, 0, 1, 0)) == _lib.VF_OK  # a million is inside the limits
    assert lib.vf_warp_frames_host(None, sa, da, wa, ha, 1, 3, ident, 0, 0, 2, zero) == _lib.VF_E_INVALID

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, w=11, h=9, channels=3, m=ident, mode=0, interp=0, border=2, value=zero):
            return lib.vf_warp_device(vf_ctx.handle, src, dstp, w, h, channels, m, mode, interp, border, value, None)

        for kwargs, word in [(dict(mode=7), b"mode=7"), (dict(interp=-1), b"interp=-1"), (dict(border=9), b"unknown border 9"),
                             (dict(m=dmap(1, nan, 0, 0, 1, 0)), b"m[1] is not finite"), (dict(channels=2), b"channels=2"),
                             (dict(w=0), b"frame"), (dict(h=-1), b"frame"), (dict(src=None), b"NULL buffer"),
                             (dict(dstp=None), b"NULL buffer"),
                             (dict(dstp=d), b"src and dst overlap"),  # not even in place: an output pixel reads anywhere
                             (dict(dstp=d + n - 1), b"src and dst overlap"), (dict(dstp=d + 1), b"src and dst overlap"),
                             # refused before any GPU work: the far destination is never touched
                             (dict(w=32768, h=1, channels=1, dstp=d + (1 << 20)), b"a side is at most 32767"),
                             (dict(w=1, h=40000, channels=1, dstp=d + (1 << 20)), b"a side is at most 32767"),
                             (dict(m=dmap(2e5, 0, 0, 0, 1, 0)), b"m[0]=200000"),
                             (dict(m=dmap(1, 0, 0, 0, 1, 1048575.5)), b"m[5]=1048575.5")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)

    # a VF_STEP_WARP step goes through the same checks; 11, 13, 4 and -1 stay no kinds
    def data(m=(1, 0, 0.5, 0, 1, 0.25), mode=0, interp=0, value=(0, 0, 0)):
        return np.frombuffer(np.array(m, np.float64).tobytes() + np.array([mode, interp, *value, 0], np.int32).tobytes(), np.uint8)

    good = data()

    def chain(kind=12, d=good, border=2, channels=3):
        st = (_lib.Step * 1)()
        st[0].kind, st[0].a, st[0].op, st[0].border = kind, 0, 0, border
        st[0].data = d.ctypes.data if d is not None else None
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, st, 1)

    for kwargs, word in [(dict(d=None), b"step 1: the warp step's data is NULL"),
                         (dict(d=data(mode=4)), b"step 1: mode=4"), (dict(d=data(interp=2)), b"step 1: interp=2"),
                         (dict(d=data(value=(0, 0, 300))), b"step 1: value[2]=300"), (dict(border=3), b"step 1: unknown border 3"),
                         (dict(d=data(m=(1, 0, nan, 0, 1, 0))), b"step 1: m[2] is not finite"),
                         (dict(d=data(m=(1, 0, 0, 0, 1, 3e6))), b"frame 0: m[4]=1.000000 and m[5]=3000000"),
                         (dict(kind=11), b"unknown kind 11"), (dict(kind=13), b"unknown kind 13"),
                         (dict(kind=4), b"unknown kind 4"), (dict(kind=-1), b"unknown kind -1")]:
        assert chain(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        still_works()
    assert chain() == _lib.VF_OK and np.array_equal(dst, probe_want)
    assert chain(d=data(mode=3, interp=1)) == _lib.VF_OK and np.array_equal(dst, img[::-1, ::-1])
    still_works()
