"""CLAHE on raw frames (``vf_clahe_*``, ``vfilter.clahe``, ``create_clahe``, ``clahe_frames``) against the numpy
reference of ``tests/_clahe_ref.py``.  Every comparison is exact.

Sizes: 1 x 1 and 1 x 5 under an 8 x 8 grid and 5 x 7 have tiles of one padded pixel and a margin that
reflects more than once; 64 x 64 divides, 66 x 64 takes the full-tile pad; 250 x 130 and 135 x 241 divide on
neither axis; 3 x 300 under 16 x 1 and 97 x 53 under 1 x 1 have one tile on an axis, where both tile indices
clamp to it; 480 x 480 under 8 x 8 has tiles of 60 rows, which the histogram and the blend cut into
several workgroups each.  The references are computed once and shared.
"""
import ctypes

import numpy as np
import pytest

import _clahe_ref as R
import _level_ref as L
import vfilter
from vfilter import Clahe, _lib

pytestmark = pytest.mark.gpu

# (height, width, (tiles_x, tiles_y))
CASES = [(1, 1, (1, 1)), (1, 1, (8, 8)), (1, 5, (8, 8)), (5, 7, (8, 8)), (17, 13, (4, 2)), (64, 64, (8, 8)),
         (66, 64, (8, 8)), (250, 130, (8, 8)), (135, 241, (16, 16)), (3, 300, (16, 1)), (97, 53, (1, 1)),
         (480, 480, (8, 8))]
CONTENTS = ["random", "constant", "two_values", "ramp", "channel_constants", "tile_constants"]
LIMITS = [0, 1, 256, 512, 10240]  # clip_q8: none, 1 / 256, 1.0, 2.0, 40.0


def _frame(content, h, w, c, grid=(8, 8)):
    rng = np.random.default_rng([h, w, c, CONTENTS.index(content)])
    shape = (h, w, c) if c == 3 else (h, w)
    if content == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "constant":
        return np.full(shape, 77, np.uint8)
    if content == "two_values":
        return rng.choice(np.array([40, 201], np.uint8), shape)
    if content == "ramp":  # every channel another slope, a narrow range
        a = (np.arange(h * w, dtype=np.int64).reshape(h, w) * 3) % 150 + 30
        return a.astype(np.uint8) if c == 1 else np.stack([a, (a * 2) % 97 + 11, 255 - a], axis=2).astype(np.uint8)
    if content == "channel_constants":  # every channel another constant: a channel-phase slip shows
        a = np.empty(shape, np.uint8)
        if c == 1:
            a[:] = 9
        else:
            a[:, :, 0], a[:, :, 1], a[:, :, 2] = 9, 130, 251
        return a
    # every tile its own pair of values, so every tile its own table: a slipped tile index shows
    _, _, th, tw = R.geometry(h, w, *grid)
    ty, tx = np.arange(h)[:, None] // th, np.arange(w)[None, :] // tw
    a = ((ty * grid[0] + tx) * 7 % 200 + 20 + 30 * ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1)).astype(np.uint8)
    return a if c == 1 else np.stack([a, 255 - a, (a.astype(np.int64) * 3 % 251).astype(np.uint8)], axis=2)


_REF = {}


def _want(key, img, q, grid, mask=0):
    """The reference of a (frame, filter) pair, computed once."""
    k = (key, q, grid, mask)
    if k not in _REF:
        out = R.clahe(img, q, grid[0], grid[1], mask)
        out.flags.writeable = False
        _REF[k] = out
    return _REF[k]


def _filter(q, grid, mask=0):
    chans = None if mask == 0 else tuple(c for c in range(3) if mask >> c & 1)
    f = Clahe(q / 256, grid, chans)
    assert f.args == (q, grid[0], grid[1], mask)
    return f


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("content", CONTENTS)
def test_every_size_and_limit(vf_ctx, content, c):
    for h, w, grid in CASES:
        img = _frame(content, h, w, c, grid)
        for q in LIMITS:
            out = vfilter.clahe_frames([img], _filter(q, grid), ctx=vf_ctx)[0]
            want = _want((content, h, w, c), img, q, grid)
            assert out.shape == img.shape and np.array_equal(out, want), (h, w, grid, q, np.argwhere(out != want)[:5])


def test_the_frames_are_what_they_are_chosen_for():
    img = _frame("tile_constants", 250, 130, 1)
    tabs = R.tile_tables(img, 512, 8, 8)
    assert len({tabs[ty, tx].tobytes() for ty in range(8) for tx in range(8)}) >= 60  # nearly every tile its own table
    rnd = _frame("random", 250, 130, 1)
    outs = {q: _want(("random", 250, 130, 1), rnd, q, (8, 8)).tobytes() for q in LIMITS}
    # every limit another picture, but 40.0: 85 counts a bin, which no bin of a 17 x 32 tile of noise reaches
    assert len(set(outs.values())) == len(LIMITS) - 1 and outs[0] == outs[10240]
    flat = _frame("two_values", 250, 130, 1)
    assert not np.array_equal(R.clahe(flat, 10240), R.clahe(flat, 0))  # two bins of 272: there 40.0 clips
    assert R.geometry(66, 64, 8, 8) == (72, 72, 9, 9) and R.geometry(5, 7, 8, 8) == (8, 8, 1, 1)
    one = _frame("ramp", 97, 53, 1)  # a 1 x 1 grid with no clipping: global equalisation without the first-bin rule
    assert np.array_equal(R.clahe(one, 0, 1, 1), R.tile_tables(one, 0, 1, 1)[0, 0][one])


@pytest.mark.parametrize("mask", [0, 1, 2, 5])
def test_masks(vf_ctx, mask):
    for h, w, grid in [(17, 13, (4, 2)), (250, 130, (8, 8))]:
        img = _frame("ramp", h, w, 3)
        got = vfilter.clahe_frames([img], _filter(512, grid, mask), ctx=vf_ctx)[0]
        assert np.array_equal(got, _want(("ramp", h, w, 3), img, 512, grid, mask)), (h, w, mask)
        for ch in range(3):  # an unmasked channel passes unchanged
            if mask and not mask >> ch & 1:
                assert np.array_equal(got[:, :, ch], img[:, :, ch])
    if mask in (0, 1):
        gray = _frame("ramp", 250, 130, 1)
        assert np.array_equal(vfilter.clahe_frames([gray], _filter(512, (8, 8), mask), ctx=vf_ctx)[0],
                              _want(("ramp", 250, 130, 1), gray, 512, (8, 8)))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("so,do", [(0, 0), (1, 1), (7, 7), (15, 15), (3, 8), (0, 5), (9, 0), (15, 1)])
def test_device_buffers_off_the_16_byte_grid(vf_ctx, c, so, do):
    """Every pixel access is bytewise, so any pair of offsets runs the same code; canaries on both sides."""
    h, w, grid = 37, 171, (8, 8)
    img = _frame("ramp", h, w, c)
    n = img.nbytes
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.clahe_device(dsrc + so, ddst + 16 + do, w, h, c, 512, 8, 8, 0)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        for p in (dsrc, ddst):
            vf_ctx.free_device(p)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), _want(("ramp", h, w, c), img, 512, grid))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)


@pytest.mark.parametrize("c", [1, 3])
def test_in_place(vf_ctx, c):
    img = _frame("ramp", 250, 130, c)
    want = _want(("ramp", 250, 130, c), img, 512, (8, 8))
    buf = img.copy()
    assert vfilter.clahe(buf, 2.0, dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, want)
    n = img.nbytes
    got = np.empty_like(img)
    d = vf_ctx.alloc_device(n)
    try:
        vf_ctx.upload(d, img, n)
        vf_ctx.clahe_device(d, d, 130, 250, c, 512)  # dst is src on the device
        vf_ctx.sync()
        vf_ctx.download(got, d, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    assert np.array_equal(got, want)


def test_clahe_frames_with_mixed_sizes_and_an_empty_frame(vf_ctx):
    for c in (1, 3):
        frames = [_frame("random", 17, 13, c), np.empty((0, 0, 3) if c == 3 else (0, 0), np.uint8),
                  _frame("ramp", 250, 130, c), _frame("two_values", 1, 5, c), _frame("constant", 66, 64, c)]
        outs = vfilter.clahe_frames(frames, Clahe(2.0), ctx=vf_ctx)
        assert len(outs) == len(frames)
        for f, o in zip(frames, outs):
            assert o.shape == f.shape and np.array_equal(o, R.clahe(f, 512)), f.shape
        filled = [np.empty_like(f) for f in frames]
        assert vfilter.clahe_frames(frames, Clahe(40.0, (4, 2)), outs=filled, ctx=vf_ctx) is filled
        for f, o in zip(frames, filled):
            assert np.array_equal(o, R.clahe(f, 10240, 4, 2))
    assert vfilter.clahe_frames([], Clahe(), ctx=vf_ctx) == []


def test_two_grids_back_to_back_reuse_the_scratch(vf_ctx):
    """Stale histogram words or tables of the call before, laid out for another grid, would change the second."""
    a, b = _frame("random", 250, 130, 3), _frame("ramp", 250, 130, 3)
    first = vfilter.clahe(a, 2.0, (16, 16), ctx=vf_ctx)
    other = vfilter.clahe(b, 2.0, (4, 2), ctx=vf_ctx)
    again = vfilter.clahe(a, 2.0, (16, 16), ctx=vf_ctx)
    assert np.array_equal(first, again) and np.array_equal(first, R.clahe(a, 512, 16, 16))
    assert np.array_equal(other, R.clahe(b, 512, 4, 2))
    n = a.nbytes
    got = np.empty_like(a)
    d = vf_ctx.alloc_device(2 * n)
    try:
        for img, grid in ((a, (16, 16)), (b, (2, 3)), (a, (8, 8))):  # back to back on one stream: one scratch in order
            vf_ctx.upload(d, img, n)
            vf_ctx.clahe_device(d, d + n, 130, 250, 3, 512, grid[0], grid[1], 0)
        vf_ctx.sync()
        vf_ctx.download(got, d + n, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    assert np.array_equal(got, _want(("random", 250, 130, 3), a, 512, (8, 8)))


def test_a_frame_larger_than_the_staging():
    big = np.random.default_rng(12).integers(0, 256, (600, 700, 3), dtype=np.uint8) // 2
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for call in (lambda: vfilter.clahe(big, 2.0, ctx=ctx),
                     lambda: vfilter.chain(big, [Clahe(2.0), vfilter.filters.Invert()], ctx=ctx)):
            with pytest.raises(vfilter.VFilterError) as e:
                call()
            assert "600 rows of 2100 bytes do not fit the context's" in str(e.value) and "staging" in str(e.value)
        small = np.ascontiguousarray(big[:100])  # and the context still works, on a frame that fits
        assert np.array_equal(vfilter.clahe(small, 2.0, ctx=ctx), R.clahe(small, 512))


def test_conveniences(vf_ctx):
    img = _frame("ramp", 37, 53, 3)
    view = img[:, :, 2]  # not contiguous
    assert np.array_equal(vfilter.clahe(view, 2.0, (4, 4), ctx=vf_ctx), R.clahe(view.copy(), 512, 4, 4))
    dst = np.empty_like(img)
    assert vfilter.clahe(img, 2.5, (3, 5), channels=[0, 2], dst=dst, ctx=vf_ctx) is dst
    assert np.array_equal(dst, R.clahe(img, 640, 3, 5, 5))
    obj = vfilter.create_clahe(2.0, (8, 8), ctx=vf_ctx)  # the cv2.createCLAHE drop-in
    gray = _frame("random", 250, 130, 1)
    assert np.array_equal(obj.apply(gray), _want(("random", 250, 130, 1), gray, 512, (8, 8)))
    assert obj.getClipLimit() == 2.0 and obj.getTilesGridSize() == (8, 8)
    assert np.array_equal(vfilter.clahe(gray, ctx=vf_ctx), _want(("random", 250, 130, 1), gray, 10240, (8, 8)))  # cv2's defaults
    empty = np.empty((0, 0, 3), np.uint8)
    assert vfilter.clahe(empty, ctx=vf_ctx).shape == (0, 0, 3)
    with pytest.raises(ValueError):
        vfilter.clahe_frames([img[:, :, 0].copy()], Clahe(2.0, channels=(1,)), ctx=vf_ctx)  # channel 1 of a gray frame
    with pytest.raises(ValueError):
        vfilter.clahe(img, 0.3, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.clahe(img.astype(np.int16), ctx=vf_ctx)


def test_the_other_filters_are_unchanged_after_a_clahe_call(vf_ctx):
    img = _frame("ramp", 250, 130, 3)
    vfilter.clahe(img, 2.0, ctx=vf_ctx)
    assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), L.level(img, L.EQUALIZE))
    assert np.array_equal(vfilter.auto_levels(img, 0.01, ctx=vf_ctx), L.level(img, L.STRETCH, 0, 0, (655, 655)))
    assert np.array_equal(vfilter.calc_hist(img, ctx=vf_ctx), L.hist(img))
    assert np.array_equal(vfilter.bitwise_not(img, ctx=vf_ctx), 255 - img)
    t = np.arange(255, -1, -1).astype(np.uint8) // 2
    assert np.array_equal(vfilter.lut(img, t, ctx=vf_ctx), t[img])
    assert np.array_equal(vfilter.clahe(img, 2.0, ctx=vf_ctx), _want(("ramp", 250, 130, 3), img, 512, (8, 8)))
    # a program with a level step after one with a CLAHE step on the same context, and back
    assert np.array_equal(vfilter.chain(img, [Clahe(2.0), vfilter.Level.equalize()], ctx=vf_ctx),
                          L.level(_want(("ramp", 250, 130, 3), img, 512, (8, 8)), L.EQUALIZE))
    assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), L.level(img, L.EQUALIZE))


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _frame("ramp", 9, 11, 3)
    dst = np.empty_like(img)
    probe_want = R.clahe(img, 512, 4, 2)

    def still_works():
        assert np.array_equal(vfilter.clahe(img, 2.0, (4, 2), ctx=vf_ctx), probe_want)

    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)

    def host(q=512, tx=4, ty=2, mask=0, channels=3, srcs=sa, dsts=da, widths=wa, heights=ha, n=1):
        return lib.vf_clahe_frames_host(vf_ctx.handle, srcs, dsts, widths, heights, n, channels, q, tx, ty, mask)

    null1 = (ctypes.c_void_p * 1)(None)
    refusals = [
        (dict(q=-1), b"clip_q8=-1 outside 0..16777216"), (dict(q=(1 << 24) + 1), b"clip_q8=16777217 outside"),
        (dict(tx=0), b"tiles_x=0 outside 1..16"), (dict(tx=17), b"tiles_x=17 outside 1..16"),
        (dict(ty=0), b"tiles_y=0 outside 1..16"), (dict(ty=17), b"tiles_y=17 outside 1..16"),
        (dict(mask=8), b"channel mask 8 outside 0..7"), (dict(mask=-1), b"channel mask -1"),
        (dict(channels=2), b"channels=2"), (dict(channels=4), b"channels=4"),
        (dict(channels=1, mask=2), b"names a channel beyond the frame's 1"),
        (dict(widths=(ctypes.c_int * 1)(0)), b"frame"), (dict(heights=(ctypes.c_int * 1)(-9)), b"frame"),
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
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK
    assert lib.vf_clahe_frames_host(None, sa, da, wa, ha, 1, 3, 512, 8, 8, 0) == _lib.VF_E_INVALID

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n)
    try:
        def dev(src=d, dstp=d + n, w=11, h=9, channels=3, q=512, tx=4, ty=2, mask=0):
            return lib.vf_clahe_device(vf_ctx.handle, src, dstp, w, h, channels, q, tx, ty, mask, None)

        for kwargs, word in [(dict(q=-5), b"clip_q8=-5"), (dict(tx=33), b"tiles_x=33"), (dict(ty=-1), b"tiles_y=-1"),
                             (dict(mask=9), b"channel mask 9"), (dict(channels=2), b"channels=2"),
                             (dict(channels=1, mask=4), b"beyond the frame's 1"),
                             (dict(w=0), b"frame"), (dict(h=-1), b"frame"), (dict(src=None), b"NULL buffer"),
                             (dict(dstp=None), b"NULL buffer"), (dict(dstp=d + n - 1), b"partially overlap"),
                             (dict(w=1 << 20, h=1 << 20, channels=1), b"a frame of 1099511627776 pixels; at most 4294967295"),
                             (dict(w=65535, h=65535, channels=1, tx=1, ty=1), b"a tile of 65535 x 65535 pixels; its area")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK and dev(dstp=d) == _lib.VF_OK  # in place is allowed
        assert dev(w=0, h=0) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)

    # a VF_STEP_CLAHE step goes through the same checks; 4, 6, 9, 11 and -1 stay no kinds
    good = np.array([0, 512, 4, 2], np.int32)

    def chain(kind=10, data=good, channels=3):
        st = (_lib.Step * 1)()
        st[0].kind, st[0].a, st[0].op = kind, 0, 0
        st[0].data = data.ctypes.data if data is not None else None
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, st, 1)

    for kwargs, word in [(dict(data=None), b"step 1: the CLAHE step's data is NULL"),
                         (dict(data=np.array([8, 512, 4, 2], np.int32)), b"step 1: channel mask 8"),
                         (dict(data=np.array([0, -1, 4, 2], np.int32)), b"step 1: clip_q8=-1"),
                         (dict(data=np.array([0, 512, 17, 2], np.int32)), b"step 1: tiles_x=17"),
                         (dict(data=np.array([0, 512, 4, 0], np.int32)), b"step 1: tiles_y=0"),
                         (dict(kind=11), b"unknown kind 11"), (dict(kind=9), b"unknown kind 9"), (dict(kind=6), b"unknown kind 6"),
                         (dict(kind=4), b"unknown kind 4"), (dict(kind=-1), b"unknown kind -1")]:
        assert chain(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        still_works()
    assert chain() == _lib.VF_OK and np.array_equal(dst, probe_want)
    still_works()
