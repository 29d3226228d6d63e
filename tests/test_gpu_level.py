"""The level filter and the histogram on raw frames (``vf_hist_*``, ``vf_level_*``, ``vfilter.calc_hist``,
``equalize_hist``, ``auto_levels``, ``level_frames``) against the numpy reference of ``tests/_level_ref.py``.
Every comparison is exact.

Sizes: the stream kernels' tile is 256 lanes x 4 vectors x 16 B = 16 KiB, so 480 x 480 x 3 (675 KiB) runs
42 whole tiles and a partial one over several workgroups, 250 x 130 a few, and the small frames only
the head, tail and partial-tile paths.  ``stream::chunks`` cuts a launch only above 512 MiB of body,
which no test of a few MB reaches: that boundary is covered by ``tests/stream/stream_split_check.cc``
on the CPU, not here.  No frame here has more tiles than the grid's cap; the strided grid, a
workgroup's second and later tiles, is covered in ``tests/test_gpu_grid_stride.py``.
"""
import ctypes

import numpy as np
import pytest

import _level_ref as R
import vfilter
from vfilter import Level, _lib

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 5), (3, 1), (17, 13), (33, 17), (250, 130), (480, 480)]  # (height, width)
CONTENTS = ["random", "constant", "two_values", "ramp", "channel_constants"]
RULES = [("equalize", Level.equalize(), (R.EQUALIZE, 0, 0, (0, 0))),
         ("stretch0", Level.stretch(), (R.STRETCH, 0, 0, (0, 0))),
         ("stretch1pc", Level.stretch(0.01), (R.STRETCH, 0, 0, (655, 655))),
         ("stretch_lo_hi", Level.stretch((0.3, 0.002)), (R.STRETCH, 0, 0, (19661, 131)))]


def _frame(content, h, w, c):
    rng = np.random.default_rng([h, w, c, CONTENTS.index(content)])
    shape = (h, w, c) if c == 3 else (h, w)
    if content == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "constant":
        return np.full(shape, 77, np.uint8)
    if content == "two_values":
        return rng.choice(np.array([40, 201], np.uint8), shape)
    if content == "ramp":  # every channel another slope, a narrow range: both rules have work to do
        a = (np.arange(h * w, dtype=np.int64).reshape(h, w) * 3) % 150 + 30
        return a.astype(np.uint8) if c == 1 else np.stack([a, (a * 2) % 97 + 11, 255 - a], axis=2).astype(np.uint8)
    a = np.empty(shape, np.uint8)  # every channel another constant: a channel-phase slip shows
    if c == 1:
        a[:] = 9
    else:
        a[:, :, 0], a[:, :, 1], a[:, :, 2] = 9, 130, 251
    return a


_REF = {}


def _want(key, img, rule, mask, link, clips):
    """The reference of a (frame, filter) pair, computed once."""
    k = (key, rule, mask, link, clips)
    if k not in _REF:
        _REF[k] = R.level(img, rule, mask, link, clips)
    return _REF[k]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("content", CONTENTS)
def test_hist_and_both_rules_over_the_sizes(vf_ctx, content, c):
    for h, w in SIZES:
        img = _frame(content, h, w, c)
        got = vfilter.calc_hist(img, ctx=vf_ctx)
        assert got.dtype == np.uint32 and got.shape == (c, 256) and np.array_equal(got, R.hist(img)), (h, w)
        for name, lv, ref in RULES:
            out = vfilter.level_frames([img], lv, ctx=vf_ctx)[0]
            want = _want((content, h, w, c), img, *ref)
            assert np.array_equal(out, want), (name, h, w, np.argwhere(out != want)[:5])


def test_a_long_one_channel_row(vf_ctx):
    img = np.random.default_rng(5).integers(0, 256, (1, 100003), dtype=np.uint8)
    assert np.array_equal(vfilter.calc_hist(img, ctx=vf_ctx), R.hist(img))
    assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), R.level(img, R.EQUALIZE))
    assert np.array_equal(vfilter.auto_levels(img[:, :50001] // 3 + 20, 0.02, ctx=vf_ctx),
                          R.level(img[:, :50001] // 3 + 20, R.STRETCH, 0, 0, (1311, 1311)))


def test_a_constant_frame_past_any_16_bit_counter(vf_ctx):
    """300 x 300 = 90000 > 65535 equal bytes a channel, all from one workgroup's lanes at once in places."""
    for c in (1, 3):
        img = np.full((300, 300, c) if c == 3 else (300, 300), 200, np.uint8)
        hist = vfilter.calc_hist(img, ctx=vf_ctx)
        assert np.array_equal(hist, R.hist(img)) and int(hist[0, 200]) == 90000
        assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), img)
        img[0, 0] = 3  # no longer constant: everything else goes to 255
        assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), R.level(img, R.EQUALIZE))


@pytest.mark.parametrize("c", [1, 3])
def test_host_sources_at_every_offset_from_a_16_byte_boundary(vf_ctx, c):
    """``calc_hist`` keeps the caller's offset mod 16 in its staging, so the kernel's head and tail paths
    run at every offset; the frame is a slice of a larger buffer."""
    n = 3 * 1999  # whole pixels for both channel counts; the body's first byte changes channel with the offset
    store = np.random.default_rng(8).integers(0, 256, n + 64, dtype=np.uint8)
    base = (-store.ctypes.data) % 16
    for off in range(1, 16):
        flat = store[base + off:base + off + n]
        assert flat.ctypes.data % 16 == off
        img = flat.reshape(1, n // c, c) if c == 3 else flat.reshape(1, n)
        assert np.array_equal(vfilter.calc_hist(img, ctx=vf_ctx), R.hist(img)), off
        assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), R.level(img, R.EQUALIZE)), off


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("so,do", [(0, 0), (1, 1), (7, 7), (15, 15), (3, 8), (0, 5), (9, 0), (15, 1)])
def test_device_buffers_off_the_16_byte_grid(vf_ctx, c, so, do):
    """``so == do``: the stream kernel with a head and a tail; else the bytewise kernel.  Canaries on both sides."""
    h, w = 37, 171
    img = _frame("ramp", h, w, c)
    n = img.nbytes
    got, hist = np.empty(n + 64, np.uint8), np.empty((c, 256), np.uint32)
    dsrc, ddst, dh = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(c * 1024)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.hist_device(dsrc + so, n, c, dh)
        vf_ctx.level_device(dsrc + so, ddst + 16 + do, w, h, c, R.STRETCH, 0, 0, 655, 655)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.download(hist, dh, c * 1024)
        vf_ctx.sync()
    finally:
        for p in (dsrc, ddst, dh):
            vf_ctx.free_device(p)
    lo = 16 + do
    assert np.array_equal(hist, R.hist(img))
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), R.level(img, R.STRETCH, 0, 0, (655, 655)))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)


@pytest.mark.parametrize("c", [1, 3])
def test_in_place(vf_ctx, c):
    img = _frame("ramp", 250, 130, c)
    want = R.level(img, R.EQUALIZE)
    buf = img.copy()
    assert vfilter.equalize_hist(buf, dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, want)
    n = img.nbytes
    got = np.empty_like(img)
    d = vf_ctx.alloc_device(n)
    try:
        vf_ctx.upload(d, img, n)
        vf_ctx.level_device(d, d, 130, 250, c, R.EQUALIZE)  # dst is src on the device
        vf_ctx.sync()
        vf_ctx.download(got, d, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("link", [False, True])
@pytest.mark.parametrize("channels", [None, (0,), (1,), (2,), (0, 2), (1, 2), (0, 1, 2)])
def test_mask_subsets_and_link(vf_ctx, channels, link):
    img = _frame("ramp", 33, 17, 3)
    mask = 0 if channels is None else sum(1 << c for c in channels)
    for lv, rule, clips in ((Level.equalize(channels, link), R.EQUALIZE, (0, 0)),
                            (Level.stretch(0.05, channels, link), R.STRETCH, (3277, 3277))):
        got = vfilter.level_frames([img], lv, ctx=vf_ctx)[0]
        want = R.level(img, rule, mask, int(link), clips)
        assert np.array_equal(got, want), (channels, link, rule)
        for ch in range(3):  # an unmasked channel passes unchanged
            if mask and not mask >> ch & 1:
                assert np.array_equal(got[:, :, ch], img[:, :, ch])
    if channels in (None, (0,)):  # one channel: link changes nothing
        gray = img[:, :, 1].copy()
        assert np.array_equal(vfilter.level_frames([gray], Level.equalize(channels, link), ctx=vf_ctx)[0],
                              R.level(gray, R.EQUALIZE))


def test_level_frames_with_mixed_sizes_and_an_empty_frame(vf_ctx):
    for c in (1, 3):
        frames = [_frame("random", 17, 13, c), np.empty((0, 0, 3) if c == 3 else (0, 0), np.uint8),
                  _frame("ramp", 250, 130, c), _frame("two_values", 1, 5, c), _frame("constant", 33, 17, c)]
        outs = vfilter.level_frames(frames, Level.stretch(0.01), ctx=vf_ctx)
        hists = vfilter.calc_hist_frames(frames, ctx=vf_ctx)
        assert len(outs) == len(hists) == len(frames)
        for f, o, h in zip(frames, outs, hists):
            assert o.shape == f.shape and np.array_equal(o, R.level(f, R.STRETCH, 0, 0, (655, 655))), f.shape
            assert np.array_equal(h, R.hist(f) if f.size else np.zeros((c, 256), np.uint32)), f.shape
        filled = [np.empty_like(f) for f in frames]
        assert vfilter.level_frames(frames, Level.equalize(), outs=filled, ctx=vf_ctx) is filled
        for f, o in zip(frames, filled):
            assert np.array_equal(o, R.level(f, R.EQUALIZE))
    assert vfilter.calc_hist_frames([], ctx=vf_ctx) == []


def test_a_frame_larger_than_the_staging():
    """600 x 700 x 3 = 1.2 MiB in 1 MiB of staging: the histogram accumulates over two fills and is right; the
    filter needs the whole frame and refuses it, in words, and is never cut into bands."""
    big = np.random.default_rng(12).integers(0, 256, (600, 700, 3), dtype=np.uint8) // 2
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        assert np.array_equal(vfilter.calc_hist(big, ctx=ctx), R.hist(big))
        gray = big.reshape(600, 2100)
        assert np.array_equal(vfilter.calc_hist(gray[:, 1:], ctx=ctx), R.hist(np.ascontiguousarray(gray[:, 1:])))
        for call in (lambda: vfilter.equalize_hist(big, ctx=ctx), lambda: vfilter.auto_levels(big, 0.01, ctx=ctx),
                     lambda: vfilter.chain(big, [Level.equalize(), vfilter.filters.Invert()], ctx=ctx)):
            with pytest.raises(vfilter.VFilterError) as e:
                call()
            assert "600 rows of 2100 bytes do not fit the context's" in str(e.value) and "staging" in str(e.value)
        small = big[:100]  # and the context still works, on a frame that fits
        assert np.array_equal(vfilter.equalize_hist(np.ascontiguousarray(small), ctx=ctx), R.level(small, R.EQUALIZE))


def test_two_calls_in_a_row_give_the_same_result(vf_ctx):
    """Stale histogram words of the call before would change the second table."""
    a, b = _frame("random", 250, 130, 3), _frame("ramp", 250, 130, 3)
    first = vfilter.equalize_hist(a, ctx=vf_ctx)
    other = vfilter.equalize_hist(b, ctx=vf_ctx)
    again = vfilter.equalize_hist(a, ctx=vf_ctx)
    assert np.array_equal(first, again) and np.array_equal(first, R.level(a, R.EQUALIZE))
    assert np.array_equal(other, R.level(b, R.EQUALIZE))
    h1, h2 = vfilter.calc_hist(a, ctx=vf_ctx), vfilter.calc_hist(a, ctx=vf_ctx)
    assert np.array_equal(h1, h2) and np.array_equal(h1, R.hist(a))
    n = a.nbytes
    got = np.empty_like(a)
    d = vf_ctx.alloc_device(2 * n)
    try:
        for img in (a, b, a):  # back to back on one stream: one set of words serves them in order
            vf_ctx.upload(d, img, n)
            vf_ctx.level_device(d, d + n, 130, 250, 3, R.STRETCH, 0, 1, 655, 655)
        vf_ctx.sync()
        vf_ctx.download(got, d + n, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    assert np.array_equal(got, R.level(a, R.STRETCH, 0, 1, (655, 655)))


def test_conveniences(vf_ctx):
    img = _frame("ramp", 37, 53, 3)
    view = img[:, :, 2]  # not contiguous
    assert np.array_equal(vfilter.equalize_hist(view, ctx=vf_ctx), R.level(view.copy(), R.EQUALIZE))
    dst = np.empty_like(img)
    assert vfilter.auto_levels(img, (0.0, 0.25), link=True, dst=dst, ctx=vf_ctx) is dst
    assert np.array_equal(dst, R.level(img, R.STRETCH, 0, 1, (0, 16384)))
    empty = np.empty((0, 0, 3), np.uint8)
    assert vfilter.equalize_hist(empty, ctx=vf_ctx).shape == (0, 0, 3)
    assert not vfilter.calc_hist(empty, ctx=vf_ctx).any()
    with pytest.raises(ValueError):
        vfilter.level_frames([img[:, :, 0].copy()], Level.equalize((1,)), ctx=vf_ctx)  # channel 1 of a gray frame
    with pytest.raises(ValueError):
        vfilter.auto_levels(img, 0.5, ctx=vf_ctx)
    with pytest.raises(ValueError):
        vfilter.equalize_hist(img.astype(np.int16), ctx=vf_ctx)


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _frame("ramp", 9, 11, 3)
    dst = np.empty_like(img)
    probe_want = R.level(img, R.EQUALIZE)

    def still_works():
        assert np.array_equal(vfilter.equalize_hist(img, ctx=vf_ctx), probe_want)

    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(11), (ctypes.c_int * 1)(9)

    def host(rule=1, mask=0, link=0, lo=0, hi=0, channels=3, srcs=sa, dsts=da, widths=wa, heights=ha, n=1):
        return lib.vf_level_frames_host(vf_ctx.handle, srcs, dsts, widths, heights, n, channels, rule, mask, link, lo, hi)

    null1 = (ctypes.c_void_p * 1)(None)
    refusals = [
        (dict(rule=2), b"unknown level rule 2"), (dict(rule=-1), b"unknown level rule -1"),
        (dict(mask=8), b"channel mask 8 outside 0..7"), (dict(mask=-1), b"channel mask -1"),
        (dict(link=2), b"link=2"), (dict(link=-1), b"link=-1"),
        (dict(lo=32768), b"clips 32768, 0 outside 0..32767"), (dict(hi=-1), b"clips 0, -1 outside"),
        (dict(rule=0, lo=1), b"the equalize rule takes no clips"), (dict(rule=0, hi=9), b"the equalize rule takes no clips"),
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
    assert host() == _lib.VF_OK and np.array_equal(dst, R.level(img, R.STRETCH))
    assert host(widths=(ctypes.c_int * 1)(0), heights=(ctypes.c_int * 1)(0)) == _lib.VF_OK
    assert lib.vf_level_frames_host(None, sa, da, wa, ha, 1, 3, 0, 0, 0, 0, 0) == _lib.VF_E_INVALID

    hists = np.zeros((1, 3, 256), np.uint32)
    na = (ctypes.c_size_t * 1)(img.nbytes)

    def hist(srcs=sa, nbytes=na, n=1, channels=3, out=hists.ctypes.data):
        return lib.vf_hist_frames_host(vf_ctx.handle, srcs, nbytes, n, channels, out)

    for kwargs, word in [(dict(channels=2), b"channels=2"), (dict(nbytes=(ctypes.c_size_t * 1)(100)), b"not whole 3-channel pixels"),
                         (dict(srcs=null1), b"NULL buffer"), (dict(out=None), b"NULL array"), (dict(n=-2), b"n < 0"),
                         (dict(nbytes=None), b"NULL array")]:
        assert hist(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        still_works()
    assert hist() == _lib.VF_OK and np.array_equal(hists[0], R.hist(img))
    assert hist(n=0) == _lib.VF_OK

    n = img.nbytes
    d = vf_ctx.alloc_device(2 * n + 4096)
    try:
        def dev(src=d, dstp=d + n, w=11, h=9, channels=3, rule=0, mask=0, link=0, lo=0, hi=0):
            return lib.vf_level_device(vf_ctx.handle, src, dstp, w, h, channels, rule, mask, link, lo, hi, None)

        for kwargs, word in [(dict(rule=3), b"unknown level rule 3"), (dict(mask=9), b"channel mask 9"), (dict(link=5), b"link=5"),
                             (dict(lo=3), b"takes no clips"), (dict(rule=1, hi=40000), b"clips 0, 40000"),
                             (dict(channels=2), b"channels=2"), (dict(channels=1, mask=4), b"beyond the frame's 1"),
                             (dict(w=0), b"frame"), (dict(h=-1), b"frame"), (dict(src=None), b"NULL buffer"),
                             (dict(dstp=None), b"NULL buffer"), (dict(dstp=d + n - 1), b"partially overlap"),
                             (dict(w=1 << 20, h=1 << 20, channels=1), b"a frame of 1099511627776 pixels; at most 4294967295"),
                             (dict(w=1 << 16, h=1 << 15, link=1), b"linked channels of 2147483648 pixels")]:
            assert dev(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dev() == _lib.VF_OK and dev(dstp=d) == _lib.VF_OK  # in place is allowed
        assert dev(w=0, h=0) == _lib.VF_OK
        dh = d + 2 * n + (-(d + 2 * n)) % 16

        def dhist(src=d, nbytes=n, channels=3, out=dh):
            return lib.vf_hist_device(vf_ctx.handle, src, nbytes, channels, out, None)

        for kwargs, word in [(dict(channels=0), b"channels=0"), (dict(nbytes=n - 1), b"not whole 3-channel pixels"),
                             (dict(out=None), b"hist is NULL"), (dict(out=dh + 2), b"not 4-byte aligned"),
                             (dict(src=None), b"NULL buffer"),
                             (dict(nbytes=1 << 33, channels=1), b"a frame of 8589934592 pixels")]:
            assert dhist(**kwargs) == _lib.VF_E_INVALID, kwargs
            assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
            still_works()
        assert dhist() == _lib.VF_OK and dhist(nbytes=0, src=None) == _lib.VF_OK
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)

    # a VF_STEP_LEVEL step goes through the same checks; 4, 6 and 9 stay no kinds
    good = np.array([0, 0, 0, 0], np.int32)

    def chain(kind=8, data=good, op=0, channels=3):
        st = (_lib.Step * 1)()
        st[0].kind, st[0].a, st[0].op = kind, 0, op
        st[0].data = data.ctypes.data if data is not None else None
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, st, 1)

    for kwargs, word in [(dict(data=None), b"step 1: the level step's data is NULL"), (dict(op=2), b"step 1: unknown level rule 2"),
                         (dict(data=np.array([8, 0, 0, 0], np.int32)), b"channel mask 8"),
                         (dict(data=np.array([0, 3, 0, 0], np.int32)), b"link=3"),
                         (dict(data=np.array([0, 0, 5, 0], np.int32)), b"takes no clips"),
                         (dict(op=1, data=np.array([0, 0, 0, 32768], np.int32)), b"clips 0, 32768"),
                         (dict(kind=9), b"unknown kind 9"), (dict(kind=6), b"unknown kind 6"), (dict(kind=4), b"unknown kind 4")]:
        assert chain(**kwargs) == _lib.VF_E_INVALID, kwargs
        assert word in lib.vf_last_error(None), (kwargs, lib.vf_last_error(None))
        still_works()
    assert chain() == _lib.VF_OK and np.array_equal(dst, probe_want)
    still_works()
