"""Filter chains that hold a resize step, bit for bit: the resize is ``tests/_resize_ref.py``'s, the steps around it
are the library's single filters (each checked against its own reference elsewhere) applied to that reference's
result, so what is under test is the chain: every value has a size of its own, a resize never runs in place, and
the result has ``Chain.out_size``'s size.  Frames of 13 x 17 and 160 x 48 (W x H), alone and in a mixed batch.
"""
import numpy as np
import pytest

import _resize_ref as R
import vfilter
from vfilter import Resize
from vfilter.filters import Chain, Combine, Invert, Rank

pytestmark = pytest.mark.gpu

SHAPES = [(17, 13, 3), (48, 160, 3), (35, 67, 1)]  # (h, w, c)


def _frame(shape):
    return np.random.default_rng(list(shape)).integers(0, 256, shape if shape[2] == 3 else shape[:2], dtype=np.uint8)


def _rs(img, f):
    return R.resize(img, f.dsize, f.fx, f.fy, f.interp_code)


HALF = Resize(fx=0.5, fy=0.5)                         # linear; an even frame runs it as area 2 x 2
THIRD_N = Resize(fx=1 / 3, fy=0.5, interpolation="nearest")
UP = Resize(fx=1.5, fy=2.0)
TO_40x30 = Resize((40, 30))
TO_40x30_N = Resize((40, 30), interpolation="nearest")


def _back(img):
    return Resize((img.shape[1], img.shape[0]))


# name -> (the chain for a frame, the composition that gives its result from the reference)
PROGRAMS = {
    "shrink_median_back": (lambda img: Chain([HALF, Rank.median(3), _back(img)]),
                           lambda img, ctx: _rs(vfilter.median_blur(_rs(img, HALF), 3, ctx=ctx), _back(img))),
    "resize_first": (lambda img: Chain([UP, Invert()]), lambda img, ctx: 255 - _rs(img, UP)),
    "resize_last": (lambda img: Chain([Invert(), THIRD_N]), lambda img, ctx: _rs(255 - img, THIRD_N)),
    "resize_only": (lambda img: Chain(TO_40x30), lambda img, ctx: _rs(img, TO_40x30)),
    "two_resizes": (lambda img: Chain([UP, HALF]), lambda img, ctx: _rs(_rs(img, UP), HALF)),
    # two values resized to one size, from one frame: value 0 is read twice
    "absdiff_of_two_resizes": (lambda img: Chain(Combine("absdiff", TO_40x30, TO_40x30_N)),
                               lambda img, ctx: np.abs(_rs(img, TO_40x30).astype(np.int16) - _rs(img, TO_40x30_N)).astype(np.uint8)),
    "median_of_the_small_against_the_small": (
        lambda img: Chain.program([(HALF, 0), (Rank.median(3), 1), ("subtract", 1, 2)]),
        lambda img, ctx: np.clip(_rs(img, HALF).astype(np.int16) - vfilter.median_blur(_rs(img, HALF), 3, ctx=ctx), 0, 255).astype(np.uint8)),
}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_the_programs(vf_ctx, name):
    build, ref = PROGRAMS[name]
    frames = [_frame(s) for s in SHAPES]
    wants = [ref(img, vf_ctx) for img in frames]
    for img, want in zip(frames, wants):
        c = build(img)
        assert c.has_resize and any(st[0] == 14 for st in c.steps)
        assert c.out_size(img.shape[1], img.shape[0]) == (want.shape[1], want.shape[0])
        channels = 1 if img.ndim == 2 else 3
        assert vf_ctx.chain_out_size(c.steps, channels, img.shape[1], img.shape[0]) == (want.shape[1], want.shape[0])
        out = vfilter.chain(img, c, ctx=vf_ctx)
        assert out.shape == want.shape and np.array_equal(out, want), (name, img.shape, np.argwhere(out != want)[:5])
        given = np.empty(want.shape, np.uint8)
        assert vfilter.chain(img, c, given, ctx=vf_ctx) is given and np.array_equal(given, want)
    if name != "shrink_median_back":  # one chain for every frame: frames of mixed sizes in one call
        three = [f for f in frames if f.ndim == 3] + [np.zeros((0, 0, 3), np.uint8)]
        c = build(three[0])
        outs = vfilter.chain_frames(three, c, ctx=vf_ctx)
        assert outs[-1].shape == (0, 0, 3)
        for img, out in zip(three[:-1], outs):
            assert np.array_equal(out, ref(img, vf_ctx)), (name, img.shape)


def test_a_middle_value_larger_than_the_frame_with_several_frames_in_one_fill():
    """Up, median, down: value 2 is four times the frame.  Five frames of 192,000 bytes share one fill of a 1 MiB
    staging, each at its upload offset, so a value that reused the upload slot (buffer 0) would write over the
    frames behind it and, from the third frame on, past the staging's end: under a resize step buffer 0 holds the
    frame alone, and every later value a scratch buffer of its own."""
    frames = [np.random.default_rng([320, 200, i]).integers(0, 256, (200, 320, 3), dtype=np.uint8) for i in range(5)]
    up, down = Resize(fx=2, fy=2, interpolation="nearest"), Resize((320, 200))
    c = Chain([up, Rank.median(3), down])
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        assert 5 * frames[0].nbytes <= 1 << 20 < 2 * frames[0].nbytes + 4 * frames[0].nbytes  # one fill; the third value 2 would not fit
        outs = vfilter.chain_frames(frames, c, ctx=ctx)
        for img, out in zip(frames, outs):
            want = _rs(vfilter.median_blur(_rs(img, up), 3, ctx=ctx), down)
            assert out.shape == img.shape and np.array_equal(out, want)
        again = vfilter.chain_frames(frames, c, ctx=ctx)  # and the frames behind the first were not written over
        assert all(np.array_equal(a, b) for a, b in zip(again, outs))


def test_in_place_where_the_sizes_are_equal(vf_ctx):
    img = _frame(SHAPES[1])
    c = PROGRAMS["shrink_median_back"][0](img)
    want = PROGRAMS["shrink_median_back"][1](img, vf_ctx)
    buf = img.copy()
    assert vfilter.chain(buf, c, buf, ctx=vf_ctx) is buf and np.array_equal(buf, want)


def test_refusals(vf_ctx):
    img = _frame(SHAPES[1])
    probe = _rs(img, TO_40x30)
    unequal = Chain(Combine("absdiff", None, HALF))
    with pytest.raises(ValueError, match="chain: step 2: operand a .value 0. is 160 x 48 and operand b .value 1. is 80 x 24"):
        unequal.out_size(160, 48)
    with pytest.raises(ValueError, match="a binary step's operands have one size"):
        vfilter.chain(img, unequal, ctx=vf_ctx)
    lib_steps = unequal.steps
    with pytest.raises(vfilter.VFilterError, match="frame 0: step 2: operand a .value 0. is 160 x 48 and operand b .value 1. is 80 x 24"):
        vf_ctx.chain_frames_host([img], [np.empty_like(img)], [160], [48], 3, lib_steps)
    with pytest.raises(vfilter.VFilterError, match="step 2: operand a"):
        vf_ctx.chain_out_size(lib_steps, 3, 160, 48)
    with pytest.raises(ValueError, match="result's shape"):
        vfilter.chain(img, Chain(TO_40x30), np.empty_like(img), ctx=vf_ctx)
    with pytest.raises(ValueError, match="result's shape"):
        vfilter.chain_frames([img], Chain(TO_40x30), [np.empty_like(img)], ctx=vf_ctx)
    with pytest.raises(vfilter.VFilterError, match="frame 0: step 2: area from 80 x 24 to 30 x 10"):
        vfilter.chain(img, [HALF, Resize((30, 10), interpolation="area")], ctx=vf_ctx)
    with pytest.raises(vfilter.VFilterError, match="overlap"):  # a result of another size inside the source's memory
        vf_ctx.chain_frames_host([img], [img.reshape(-1)[:40 * 30 * 3]], [160], [48], 3, Chain(TO_40x30).steps)
    assert np.array_equal(vfilter.chain(img, Chain(TO_40x30), ctx=vf_ctx), probe)  # and the context still works

