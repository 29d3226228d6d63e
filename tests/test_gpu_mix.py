"""The colour matrix on raw frames (``vfilter.transform``, ``transform_frames``, ``vf_mix_device``,
``vf_mix_frames_host``) against the numpy reference of ``tests/_mix_ref.py``, bit for bit.

The matrix set is ``_mix_ref.matrix_set()`` plus every ``vfilter.colors`` preset, each under both
roundings where ``shift > 0``.  The frames run from one pixel over one 48-byte unit of the kernel
(16 pixels) minus and plus a pixel to 250 x 130.  The device test moves ``dst`` over all 16 offsets
mod 16 with ``src`` at the same offset, at +1 and at +7, on lengths of one tile, one tile minus and
plus a pixel and two tiles plus 5 pixels -- the tile size read from the library -- between guard
bands of 64 bytes.
"""
import ctypes

import numpy as np
import pytest

import _mix_ref as M
import _rank_ref as R
import vfilter
from vfilter import Mix, _lib, colors

pytestmark = pytest.mark.gpu

ROUNDINGS = ("half_even", "half_up")
CODE = {"half_even": 0, "half_up": 1}
# (h, w): 1, 5, 15, 16, 17 pixels in a row (one unit of 16 pixels -+ a pixel), odd sizes, several tiles
SHAPES = [(1, 1), (1, 5), (1, 15), (1, 16), (1, 17), (2, 3), (13, 17), (130, 250)]
GUARD = 64


def _plain(v):
    if isinstance(v, Mix):
        return v.matrix.astype(np.int64), v.shift
    return np.asarray(v[0], np.int64), v[1]


def _matrices():
    out = dict(M.matrix_set())
    for name, v in {"identity": colors.identity(), "swap_rb": colors.swap_rb(), "gray": colors.gray(),
                    "gray_weights14": colors.gray_weights(1868, 9617, 4899, 14), "sepia": colors.sepia(),
                    "saturation_half": colors.saturation(0.5), "saturation_1.75": colors.saturation(1.75),
                    "gain": colors.gain(1, 1.5, 0.75), "offset": colors.offset(-20, 0, 255)}.items():
        out["colors." + name] = _plain(v)
    return out


MATRICES = _matrices()
_FRAMES = {s: np.random.default_rng(100 + i).integers(0, 256, s + (3,), dtype=np.uint8) for i, s in enumerate(SHAPES)}
_FRAMES[(16, 16)] = M.tie_frame()
_WANT = {}


def _want(name, shape, rounding):
    """The reference's result, computed once and shared (never written to)."""
    key = (name, shape, rounding)
    if key not in _WANT:
        m, s = MATRICES[name]
        out = M.mix(_FRAMES[shape], m, s, rounding)
        out.flags.writeable = False
        _WANT[key] = out
    return _WANT[key]


def _cases(name):
    return ROUNDINGS if MATRICES[name][1] > 0 else ("half_even",)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_every_matrix_on_every_frame(vf_ctx, name):
    m, s = MATRICES[name]
    for rounding in _cases(name):
        for shape, img in _FRAMES.items():
            keep = img.copy()
            got = vfilter.transform(img, (m, s), rounding=rounding, ctx=vf_ctx)
            want = _want(name, shape, rounding)
            assert got.shape == img.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (name, rounding, shape, np.argwhere(got != want)[:5])
            assert np.array_equal(img, keep)
    if s == 0:  # nothing to round: half_up is the same picture
        img = _FRAMES[(13, 17)]
        assert np.array_equal(vfilter.transform(img, (m, s), rounding="half_up", ctx=vf_ctx), _want(name, (13, 17), "half_even"))


def test_the_roundings_differ_on_the_tie_frame_and_the_presets_do_what_they_say(vf_ctx):
    img = _FRAMES[(16, 16)]
    he = vfilter.transform(img, M.TIES, ctx=vf_ctx)
    hu = vfilter.transform(img, M.TIES, rounding="half_up", ctx=vf_ctx)
    assert not np.array_equal(he, hu)
    big = _FRAMES[(130, 250)]
    assert np.array_equal(vfilter.transform(big, colors.identity(), ctx=vf_ctx), big)
    assert np.array_equal(vfilter.transform(big, colors.swap_rb(), ctx=vf_ctx), big[..., ::-1])
    g = vfilter.transform(big, colors.gray(), ctx=vf_ctx)  # a Mix keeps its own rounding
    assert np.array_equal(g, _want("colors.gray", (130, 250), "half_up"))
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
    f = np.array([[0.5, 0.25, 0, 1.5], [0, 1, 0, 0], [-1, 0, 1, 0]])  # a dyadic float matrix
    assert np.array_equal(vfilter.transform(big, f, ctx=vf_ctx), M.mix(big, M.mat([[2, 1, 0], [0, 4, 0], [-4, 0, 4]], (6, 0, 0)), 2))


def test_dst_is_src(vf_ctx):
    for shape in [(1, 5), (1, 17), (13, 17), (130, 250)]:
        for name, rounding in (("colors.sepia", "half_even"), ("colors.gray", "half_up"), ("shift0_offsets", "half_even")):
            buf = _FRAMES[shape].copy()
            assert vfilter.transform(buf, MATRICES[name], dst=buf, rounding=rounding, ctx=vf_ctx) is buf
            assert np.array_equal(buf, _want(name, shape, rounding)), (name, shape)
    dst = np.empty_like(_FRAMES[(13, 17)])
    assert vfilter.transform(_FRAMES[(13, 17)], colors.sepia(), dst=dst, ctx=vf_ctx) is dst
    with pytest.raises(ValueError, match="dst must be"):
        vfilter.transform(_FRAMES[(13, 17)], colors.sepia(), dst=np.empty((13, 17), np.uint8), ctx=vf_ctx)


def test_a_mixed_size_batch(vf_ctx):
    shapes = list(SHAPES)
    frames = [_FRAMES[s] for s in shapes] + [np.empty((0, 0, 3), np.uint8)]
    for name, rounding in (("colors.sepia", "half_even"), ("colors.gray", "half_up"), ("sum_65536_shift_16", "half_even")):
        mix = Mix(MATRICES[name], rounding)
        outs = vfilter.transform_frames(frames, mix, ctx=vf_ctx)
        assert len(outs) == len(frames) and outs[-1].shape == (0, 0, 3)
        for s, o in zip(shapes, outs):
            assert np.array_equal(o, _want(name, s, rounding)), (name, s)
    bufs = [f.copy() for f in frames]  # in place, through outs
    assert vfilter.transform_frames(bufs, Mix(colors.sepia()), outs=bufs, ctx=vf_ctx)[0] is bufs[0]
    for s, o in zip(shapes, bufs):
        assert np.array_equal(o, _want("colors.sepia", s, "half_even")), s
    with pytest.raises(ValueError, match="H x W x 3"):
        vfilter.transform_frames([_FRAMES[(13, 17)][..., 0].copy()], Mix(colors.sepia()), ctx=vf_ctx)


def test_every_dst_offset_with_guard_bands(vf_ctx):
    """Device buffers from the context's allocator (``vf_alloc_device``), as ``test_gpu_binary.py``'s: a
    torch tensor cannot be made in this process, where torch finds no HIP device once the library
    holds it."""
    ctx = vf_ctx
    tile = ctx.mix_tile_bytes()
    assert tile % 48 == 0 and tile >= 48 and tile == _lib.load_library().vf_mix_tile_bytes()
    lengths = [tile, tile - 3, tile + 3, 2 * tile + 15]
    cap = max(lengths) + 2 * GUARD + 64
    dsrc, ddst = ctx.alloc_device(cap), ctx.alloc_device(cap)
    try:
        assert dsrc % 16 == 0 and ddst % 16 == 0
        rng = np.random.default_rng(48)
        data = rng.integers(0, 256, max(lengths), dtype=np.uint8)
        forms = [("colors.sepia", "half_even"), ("colors.gray", "half_up"), ("shift0_offsets", "half_even")]
        wants = {(f, n): M.mix(data[:n].reshape(-1, 3), *MATRICES[f[0]], f[1]).reshape(-1) for f in forms for n in lengths}
        got = np.empty(cap, np.uint8)
        k = 0
        for off in range(16):
            for delta in (0, 1, 7):
                for n in lengths:
                    name, rounding = form = forms[k % len(forms)]
                    k += 1
                    m, s = MATRICES[name]
                    so, lo = GUARD + off + delta, GUARD + off
                    ctx.memset_device(ddst, 0xEE, cap)
                    ctx.upload(dsrc + so, data, n)
                    ctx.mix_device(dsrc + so, ddst + lo, n, m.astype(np.int32), s, CODE[rounding])
                    ctx.download(got, ddst, cap)
                    ctx.sync()
                    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE), (off, delta, n)
                    assert np.array_equal(got[lo:lo + n], wants[form, n]), (off, delta, n, name)
        # in place at an odd offset, and the arguments the entry point itself refuses
        n, so = lengths[3], GUARD + 5
        m, s = MATRICES["colors.sepia"]
        ctx.memset_device(dsrc, 0xEE, cap)
        ctx.upload(dsrc + so, data, n)
        ctx.mix_device(dsrc + so, dsrc + so, n, m.astype(np.int32), s, 0)
        ctx.download(got, dsrc, cap)
        ctx.sync()
        assert np.all(got[:so] == 0xEE) and np.all(got[so + n:] == 0xEE)
        assert np.array_equal(got[so:so + n], wants[("colors.sepia", "half_even"), n])
        with pytest.raises(vfilter.VFilterError, match="whole 3-channel pixels"):
            ctx.mix_device(dsrc, ddst, 16, m.astype(np.int32), s, 0)
        with pytest.raises(vfilter.VFilterError, match="partially overlap"):
            ctx.mix_device(dsrc, dsrc + 3, 48, m.astype(np.int32), s, 0)
        ctx.mix_device(0, 0, 0, m.astype(np.int32), s, 0)  # nothing to do
    finally:
        ctx.sync()
        ctx.free_device(dsrc)
        ctx.free_device(ddst)


def test_the_stride_form_gives_the_same_bytes(vf_ctx, monkeypatch):
    """``VF_MIX_FORM=stride`` (read per launch) runs whole tiles in the form the partial tile always
    takes: every lane its own 48-byte units.  250 x 130 pixels are four tiles."""
    monkeypatch.setenv("VF_MIX_FORM", "stride")
    for name, rounding in (("colors.sepia", "half_even"), ("colors.gray", "half_up"), ("all_negative_row", "half_even"),
                           ("shift0_offsets", "half_even")):
        for shape in [(1, 17), (130, 250)]:
            got = vfilter.transform(_FRAMES[shape], MATRICES[name], rounding=rounding, ctx=vf_ctx)
            assert np.array_equal(got, _want(name, shape, rounding)), (name, shape)
        buf = _FRAMES[(130, 250)].copy()
        assert vfilter.transform(buf, MATRICES[name], dst=buf, rounding=rounding, ctx=vf_ctx) is buf
        assert np.array_equal(buf, _want(name, (130, 250), rounding)), (name, "in place")


def test_a_frame_larger_than_the_staging():
    big = np.random.default_rng(5).integers(0, 256, (800, 1024, 3), dtype=np.uint8)
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for name, rounding in (("colors.sepia", "half_even"), ("colors.gray", "half_up")):
            want = M.mix(big, *MATRICES[name], rounding)
            got = vfilter.transform(big, MATRICES[name], rounding=rounding, ctx=ctx)
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
            buf = big.copy()
            assert vfilter.transform(buf, MATRICES[name], dst=buf, rounding=rounding, ctx=ctx) is buf
            assert np.array_equal(buf, want), (name, "in place", np.argwhere(buf != want)[:5])


def test_every_refusal_through_the_c_abi_leaves_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _FRAMES[(13, 17)]
    dst = np.empty_like(img)
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(17), (ctypes.c_int * 1)(13)
    good = np.ascontiguousarray(MATRICES["colors.sepia"][0], np.int32)

    def mat(**kw):
        m = good.copy()
        for (c, k), v in kw.get("set", {}).items():
            m[c, k] = v
        return m

    def host(m, shift=8, rounding=0, channels=3):
        return lib.vf_mix_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, None if m is None else m.ctypes.data,
                                      shift, rounding)

    def step(m, shift=8, rounding=0, channels=3):
        arr = (_lib.Step * 1)(_lib.Step(kind=5, a=0, op=rounding, data=None if m is None else m.ctypes.data, shift=shift))
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, arr, 1)

    def still_works():
        assert np.array_equal(vfilter.transform(img, colors.sepia(), ctx=vf_ctx), _want("colors.sepia", (13, 17), "half_even"))

    wide = mat(set={(0, 0): 32768})
    heavy = mat(set={(1, 0): 32767, (1, 1): 32767, (1, 2): 3})
    far = mat(set={(2, 3): 255 * 256 + 1})
    refusals = [
        (dict(m=None), b"matrix is NULL"), (dict(m=good, shift=17), b"shift=17 outside 0..16"),
        (dict(m=good, shift=-1), b"shift=-1 outside 0..16"), (dict(m=wide), b"does not fit int16"),
        (dict(m=mat(set={(2, 2): -32769})), b"does not fit int16"), (dict(m=heavy), b"sum|M| = 65537 exceeds 65536"),
        (dict(m=far), b"at most 255 * 2^shift"), (dict(m=mat(set={(0, 3): -255 * 256 - 1})), b"at most 255 * 2^shift"),
        (dict(m=good, rounding=2), b"unknown rounding 2"), (dict(m=good, rounding=-1), b"unknown rounding -1"),
        (dict(m=good, channels=1), b"a colour matrix on 1-channel frames"),
    ]
    for call in (host, step):
        for kw, word in refusals:
            assert call(**kw) == _lib.VF_E_INVALID, (call.__name__, word)
            assert word in lib.vf_last_error(None), (call.__name__, word, lib.vf_last_error(None))
            assert word in lib.vf_last_error(vf_ctx.handle)
            still_works()
    # kind 4 names no step, now as before
    arr = (_lib.Step * 1)(_lib.Step(kind=4, a=0, data=good.ctypes.data, shift=8))
    assert lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, 3, arr, 1) == _lib.VF_E_INVALID
    assert b"unknown kind 4" in lib.vf_last_error(None)
    # the same calls with nothing wrong
    assert host(good) == _lib.VF_OK and np.array_equal(dst, _want("colors.sepia", (13, 17), "half_even"))
    dst[:] = 0
    assert step(good) == _lib.VF_OK and np.array_equal(dst, _want("colors.sepia", (13, 17), "half_even"))
    limit = mat(set={(2, 3): 255 * 256, (0, 3): -255 * 256})  # the bound itself is allowed
    assert host(limit) == _lib.VF_OK and np.array_equal(dst, M.mix(img, limit, 8))
    assert lib.vf_mix_frames_host(vf_ctx.handle, None, None, None, None, 0, 3, good.ctypes.data, 8, 0) == _lib.VF_OK
    with pytest.raises(vfilter.VFilterError, match="a colour matrix on 1-channel frames"):
        vf_ctx.mix_frames_host([img[..., 0].copy()], [dst[..., 0].copy()], [17], [13], 1, good, 8, 0)
    still_works()


def test_the_other_filters_are_undisturbed_after_a_mix(vf_ctx):
    img = _FRAMES[(130, 250)]
    assert np.array_equal(vfilter.transform(img, colors.sepia(), ctx=vf_ctx), _want("colors.sepia", (130, 250), "half_even"))
    r7 = R.element_set()["random7"]
    assert np.array_equal(vfilter.erode(img, r7, ctx=vf_ctx), R.erode(img, r7))
    assert np.array_equal(vfilter.median_blur(img, 3, ctx=vf_ctx), R.median(img, 3))
    t = vfilter.tables.gamma(2.2)
    assert np.array_equal(vfilter.lut(img, t, ctx=vf_ctx), t[img])
    assert np.array_equal(vfilter.bitwise_not(img, ctx=vf_ctx), 255 - img)
    assert np.array_equal(vfilter.transform(img, colors.gray(), ctx=vf_ctx), _want("colors.gray", (130, 250), "half_up"))
