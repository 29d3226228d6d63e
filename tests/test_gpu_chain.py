"""Filter chains on raw frames (``vf_chain_frames_host``, ``vfilter.chain``, ``chain_frames``,
``morphology_ex``) against the numpy interpreter of ``tests/_chain_ref.py``.  Every comparison is
exact.

The frames: 1 x 1 x 3 (the smallest), 3 x 2 x 3 (shorter than every reach), 17 x 13 with one and
three channels (odd sizes) and 250 x 130 x 3 (W x H: 750 row bytes are three 256-byte tiles, 130
rows nine 16-row tiles), all seeded noise.  The band test gives a 1024 x 800 x 3 frame a staging
of 1 MiB, which holds 341 rows: three bands for ``edges`` (R = 2: rows end at 339, 676, 800) and
for ``blackhat3_it2`` (R = 4: 337, 670, 800).
"""
import ctypes

import numpy as np
import pytest

import _chain_ref as CR
import _conv_ref
import _rank_ref as R
import vfilter
from _chain_build import to_chain
from vfilter import _lib, elements
from vfilter.filters import Chain, Combine, Invert, Kernel, Morph, Rank, Table

pytestmark = pytest.mark.gpu

NAMES = sorted(CR.program_set())
# (h, w, c)
SHAPES = [(1, 1, 3), (2, 3, 3), (13, 17, 1), (13, 17, 3), (130, 250, 3)]
_FRAMES = {s: CR.noise(*s) for s in SHAPES}
_WANT = {}


def _want(name, shape, border="constant"):
    """The reference's result, computed once and shared (never written to)."""
    key = (name, shape, border)
    if key not in _WANT:
        out = CR.run(_FRAMES[shape], CR.program_set(border, shape[2])[name])
        out.flags.writeable = False
        _WANT[key] = out
    return _WANT[key]


def test_the_inputs_are_not_degenerate():
    img = _FRAMES[(13, 17, 3)]
    assert not _want("gradient_corner5", (13, 17, 3)).any()  # identically zero: see tests/test_chain_ref.py
    for out in (_want("corner5_reversed", (13, 17, 3)), CR.binary("subtract", img, CR.noise(13, 17, 3, seed=1))):
        assert (out == 0).any() and (out != 0).any()
    for name in NAMES:
        if name != "gradient_corner5":
            assert _want(name, (130, 250, 3)).any() and len(np.unique(_want(name, (130, 250, 3)))) > 1, name


@pytest.mark.parametrize("name", NAMES)
def test_every_program_on_every_frame(vf_ctx, name):
    for shape in SHAPES:
        img = _FRAMES[shape]
        keep = img.copy()
        c = to_chain(CR.program_set("constant", shape[2])[name])
        got = vfilter.chain(img, c, ctx=vf_ctx)
        want = _want(name, shape)
        assert got.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)


@pytest.mark.parametrize("name", NAMES)
def test_mixed_sizes_in_one_call(vf_ctx, name):
    shapes = [s for s in SHAPES if s[2] == 3]
    frames = [_FRAMES[s] for s in shapes] + [np.empty((0, 0, 3), np.uint8)]
    c = to_chain(CR.program_set("constant", 3)[name])
    outs = vfilter.chain_frames(frames, c, ctx=vf_ctx)
    assert len(outs) == len(frames) and outs[-1].shape == (0, 0, 3)
    for s, o in zip(shapes, outs):
        assert np.array_equal(o, _want(name, s)), (name, s)
    gray = [_FRAMES[(13, 17, 1)], _FRAMES[(13, 17, 3)][:, :5, 0].copy()]
    c1 = to_chain(CR.program_set("constant", 1)[name])
    for f, o in zip(gray, vfilter.chain_frames(gray, c1, ctx=vf_ctx)):
        assert np.array_equal(o, CR.run(f, CR.program_set("constant", 1)[name])), (name, f.shape)


def test_a_three_channel_table_on_one_channel_frames_is_refused(vf_ctx):
    c = to_chain(CR.program_set("constant", 3)["pointwise"])
    with pytest.raises(ValueError, match="3-channel table"):
        vfilter.chain(_FRAMES[(13, 17, 1)], c, ctx=vf_ctx)
    # and by the library itself
    img = _FRAMES[(13, 17, 1)]
    dst = np.empty_like(img)
    with pytest.raises(vfilter.VFilterError, match="3-channel table on 1-channel frames"):
        vf_ctx.chain_frames_host([img], [dst], [17], [13], 1, *c.args)


@pytest.mark.parametrize("border", CR.BORDERS)
@pytest.mark.parametrize("name", ["edges", "dog", "eight", "gradient_random7", "corner5_reversed"])
def test_the_other_borders(vf_ctx, name, border):
    for shape in [(2, 3, 3), (13, 17, 3)]:
        c = to_chain(CR.program_set(border, 3)[name])
        got = vfilter.chain(_FRAMES[shape], c, ctx=vf_ctx)
        assert np.array_equal(got, _want(name, shape, border)), (name, border, shape)


@pytest.mark.parametrize("border", CR.BORDERS)
@pytest.mark.parametrize("op", CR.MORPH_OPS)
def test_morphology_ex(vf_ctx, op, border):
    img = _FRAMES[(13, 17, 3)]
    for ename, it in [("rect3", 1), ("cross5", 1), ("rect3x5", 2), ("random7", 1)]:
        e = R.element_set()[ename]
        got = vfilter.morphology_ex(img, op, e, it, border=border, ctx=vf_ctx)
        assert np.array_equal(got, CR.run(img, CR.morph(op, e, it, border))), (op, border, ename, it)
    # element=None is the 3 x 3 rectangle; dst is filled and returned
    dst = np.empty_like(img)
    assert vfilter.morphology_ex(img, op, dst=dst, border=border, ctx=vf_ctx) is dst
    assert np.array_equal(dst, CR.run(img, CR.morph(op, R.rect(3), 1, border)))


def test_morphology_ex_against_the_single_filters(vf_ctx):
    img = _FRAMES[(130, 250, 3)]
    c5 = elements.cross(5)
    ero, dil = vfilter.erode(img, c5, ctx=vf_ctx), vfilter.dilate(img, c5, ctx=vf_ctx)
    assert np.array_equal(vfilter.morphology_ex(img, "erode", c5, ctx=vf_ctx), ero)
    assert np.array_equal(vfilter.morphology_ex(img, "dilate", c5, ctx=vf_ctx), dil)
    assert np.array_equal(vfilter.morphology_ex(img, "open", c5, ctx=vf_ctx), vfilter.dilate(ero, c5, ctx=vf_ctx))
    assert np.array_equal(vfilter.morphology_ex(img, "close", c5, ctx=vf_ctx), vfilter.erode(dil, c5, ctx=vf_ctx))
    grad = vfilter.morphology_ex(img, "gradient", c5, ctx=vf_ctx)
    assert np.array_equal(grad, dil - ero) and grad.any()  # erode <= dilate: no saturation here
    # the structured and the explicit form of one program agree; a list of steps is a Chain
    g3, g5 = vfilter.kernels.gaussian3(), vfilter.kernels.gaussian5()
    dog = [Combine("absdiff", Kernel(g3, "constant"), Kernel(g5, "constant")), Table(CR.gamma_table())]
    assert np.array_equal(vfilter.chain(img, dog, ctx=vf_ctx), _want("dog", (130, 250, 3)))
    edges = Chain([Rank.median(3), Morph("gradient"), Table(CR.threshold_table())])
    assert np.array_equal(vfilter.chain(img, edges, ctx=vf_ctx), _want("edges", (130, 250, 3)))
    assert np.array_equal(vfilter.chain(img, Invert(), ctx=vf_ctx), 255 - img)


def test_bands_of_a_frame_larger_than_the_staging():
    big = CR.noise(800, 1024, 3, seed=5)
    ps = CR.program_set("reflect101", 3)
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        for name in ("edges", "blackhat3_it2"):
            want = CR.run(big, ps[name])
            c = to_chain(ps[name])
            got = vfilter.chain(big, c, ctx=ctx)
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
            buf = big.copy()  # dst is src: a band's halo rows are the band before's output
            assert vfilter.chain(buf, c, dst=buf, ctx=ctx) is buf
            assert np.array_equal(buf, want), (name, "in place", np.argwhere(buf != want)[:5])
        # and a mixed batch whose small frames share a fill with nothing cut
        frames = [big[:1, :1].copy(), big[:3, :5].copy(), big[:400, :640].copy()]
        c = to_chain(ps["diamond"])
        for f, o in zip(frames, vfilter.chain_frames(frames, c, ctx=ctx)):
            assert np.array_equal(o, CR.run(f, ps["diamond"])), f.shape


def test_a_one_step_chain_is_the_single_filter_band_by_band():
    """A convolution or a rank filter runs as a program of one step, so ``chain_frames`` with that one
    step and the single filter's call give the same bytes: on a 1024 x 800 x 3 frame in 1 MiB of
    staging (three bands) and on a 7 x 5 x 1 frame, out of place and with ``dst`` the source."""
    k5 = vfilter.kernels.gaussian5()
    e35 = R.element_set()["rect3x5"]
    frames = [CR.noise(800, 1024, 3, seed=5), CR.noise(5, 7, 1, seed=7)]
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        singles = [(Kernel(k5), lambda fs, outs=None: vfilter.filter2d_frames(fs, k5, outs, ctx=ctx)),
                   (Rank.erode(e35), lambda fs, outs=None: vfilter.rank_frames(fs, Rank.erode(e35), outs, ctx=ctx))]
        for step, single in singles:
            for f in frames:
                want = single([f])[0]
                assert want.shape == f.shape and want.any() and not np.array_equal(want, f)
                got = vfilter.chain_frames([f], [step], ctx=ctx)[0]
                assert np.array_equal(got, want), (step.family, f.shape, np.argwhere(got != want)[:5])
                a, b = f.copy(), f.copy()  # dst is src: a band's halo rows are the band before's output
                assert vfilter.chain_frames([a], [step], outs=[a], ctx=ctx)[0] is a and single([b], [b])[0] is b
                assert np.array_equal(a, want) and np.array_equal(b, want), (step.family, f.shape, "in place")


def test_rows_that_do_not_fit_the_staging_raise_and_the_context_goes_on():
    # 1 MiB of staging, rows of 131,072 x 3 bytes: two rows fit, blackhat3_it2 needs 2 R + 1 = 9
    wide = CR.noise(12, 131072, 3, seed=6)
    small = _FRAMES[(13, 17, 3)]
    ps = CR.program_set()
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        with pytest.raises(vfilter.VFilterError, match="9 rows of 393216 bytes do not fit") as ei:
            vfilter.chain(wide, to_chain(ps["blackhat3_it2"]), ctx=ctx)
        assert ei.value.status == _lib.VF_E_INVALID
        with pytest.raises(vfilter.VFilterError, match="5 rows of 393216 bytes do not fit"):
            vfilter.chain(wide, to_chain(ps["edges"]), ctx=ctx)
        assert np.array_equal(vfilter.chain(small, to_chain(ps["blackhat3_it2"]), ctx=ctx), _want("blackhat3_it2", (13, 17, 3)))
        # a program without reach takes the same frame, row by row
        assert np.array_equal(vfilter.chain(wide, to_chain(ps["pointwise"]), ctx=ctx), CR.run(wide, ps["pointwise"]))


def test_the_single_filters_are_undisturbed_after_chains(vf_ctx):
    img = _FRAMES[(130, 250, 3)]
    for name in ("eight", "blackhat3_it2", "dog"):
        assert np.array_equal(vfilter.chain(img, to_chain(CR.program_set()[name]), ctx=vf_ctx), _want(name, (130, 250, 3)))
    r7 = R.element_set()["random7"]
    assert np.array_equal(vfilter.erode(img, r7, ctx=vf_ctx), R.erode(img, r7))
    k, s = _conv_ref.kernel_set()["random7"]
    assert np.array_equal(vfilter.filter2d(img, (k, s), ctx=vf_ctx), _conv_ref.filter2d(img, k, s))
    t = CR.curves_table()
    assert np.array_equal(vfilter.lut(img, t, ctx=vf_ctx), CR.table(img, t))
    assert np.array_equal(vfilter.bitwise_not(img, ctx=vf_ctx), 255 - img)


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    img = _FRAMES[(13, 17, 3)]
    dst = np.empty_like(img)
    ones = np.ones(9, np.uint8)
    zeros = np.zeros(9, np.uint8)
    w3 = np.ones(9, np.int16)
    tab = np.arange(256, dtype=np.uint8)
    sa, da = (ctypes.c_void_p * 1)(img.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data)
    wa, ha = (ctypes.c_int * 1)(17), (ctypes.c_int * 1)(13)
    S = _lib.Step

    def rank(a, data=ones, **kw):
        f = dict(kind=2, a=a, op=0, data=data.ctypes.data if data is not None else None, kw=3, kh=3, border=2)
        f.update(kw)
        return S(**f)

    def host(steps, channels=3, nsteps=None):
        arr = (S * max(len(steps), 1))(*steps)
        n = len(steps) if nsteps is None else nsteps
        return lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, channels, arr, n)

    def still_works():
        assert np.array_equal(vfilter.chain(img, Morph("gradient"), ctx=vf_ctx),
                              CR.run(img, CR.morph("gradient", R.rect(3))))

    binary = S(kind=3, a=1, b=0, op=0)
    refusals = [
        ([rank(1)], b"not an earlier value"), ([rank(0), rank(2)], b"not an earlier value"),
        ([rank(0), rank(0)], b"value 1 is read by no step"),
        ([rank(0), S(kind=3, a=1, b=2, op=0)], b"operand b = 2 is not an earlier value"),
        ([rank(0), S(kind=3, a=1, b=0, op=7)], b"unknown binary op 7"),
        ([rank(0)] + [rank(i) for i in range(1, 9)], b"9 steps"), ([], b"0 steps"),
        ([S(kind=9, a=0)], b"unknown kind 9"),
        ([rank(0, zeros), binary], b"empty element"), ([rank(0, None), binary], b"element is NULL"),
        ([rank(0, kw=4), binary], b"element"), ([rank(0, op=2), binary], b"median"), ([rank(0, border=5), binary], b"border"),
        ([S(kind=1, a=0, data=w3.ctypes.data, kw=3, kh=3, shift=17), binary], b"shift"),
        ([S(kind=1, a=0, data=None, kw=3, kh=3), binary], b"weights is NULL"),
        ([S(kind=0, a=0, data=tab.ctypes.data, channels=2)], b"channels"), ([S(kind=0, a=0, data=None, channels=1)], b"table is NULL"),
    ]
    for steps, word in refusals:
        assert host(steps) == _lib.VF_E_INVALID, word
        assert word in lib.vf_last_error(None), (word, lib.vf_last_error(None))
        assert word in lib.vf_last_error(vf_ctx.handle)
        still_works()
    assert host([rank(0), binary], channels=2) == _lib.VF_E_INVALID and b"channels" in lib.vf_last_error(None)
    assert lib.vf_chain_frames_host(vf_ctx.handle, sa, da, wa, ha, 1, 3, None, 2) == _lib.VF_E_INVALID
    assert b"steps is NULL" in lib.vf_last_error(None)
    assert host([rank(0), binary]) == _lib.VF_OK  # the same call with nothing wrong: subtract(erode x, x) == 0
    assert not dst.any()
    assert host([rank(0, op=1), binary]) == _lib.VF_OK
    assert np.array_equal(dst, R.dilate(img, R.rect(3)) - img)
    # an empty batch does nothing
    arr = (S * 1)(rank(0))
    assert lib.vf_chain_frames_host(vf_ctx.handle, None, None, None, None, 0, 3, arr, 1) == _lib.VF_OK
    still_works()
