"""Filter chains that hold a warp step, bit for bit: the warp is ``tests/_warp_ref.py``'s, the steps around it are
the library's single filters (each checked against its own reference elsewhere) applied to that reference's
result, so what is under test is the chain: a warp never runs in place, reads whole frames and keeps the order of
its neighbours.  Frames of 13 x 17 and 160 x 48 (W x H); every program runs out of place, with ``src == dst`` and
in a mixed batch.
"""
import numpy as np
import pytest

import _warp_ref as R
import vfilter
from vfilter import Separable, Warp, colors, tables, warps
from vfilter.filters import Chain, Combine, Invert, Table

pytestmark = pytest.mark.gpu

SHAPES = [(17, 13, 3), (48, 160, 3)]  # (h, w, c)
GAMMA = tables.gamma(2.2)
SHIFT = warps.translation(3, -2)  # whole pixels: absdiff with the frame itself is then exact to think about
TILT = warps.rotation((6, 8), 5.0, 1.1)


def _frame(shape):
    return np.random.default_rng(list(shape)).integers(0, 256, shape, dtype=np.uint8)


def _warp(img, f):
    return R.warp(img, f.m, f.mode, f.interp_code, f.border_code, f.value)


FLIP_H = Warp(flip="h")
W_SHIFT = Warp(SHIFT, border="constant", border_value=0)
W_TILT = Warp(TILT, border="reflect101")
W_TILT_C = Warp(TILT, interpolation="nearest", border="constant", border_value=(10, 20, 30))

# name -> (the chain, the composition that gives its result from the reference)
PROGRAMS = {
    "flip_then_blur": (lambda: Chain([FLIP_H, Separable.box(5)]),
                       lambda img, ctx: vfilter.blur(_warp(img, FLIP_H), 5, ctx=ctx)),
    "gray_then_warp_then_table": (lambda: Chain([colors.gray(), W_TILT, Table(GAMMA)]),
                                  lambda img, ctx: vfilter.lut(_warp(vfilter.transform(img, colors.gray(), ctx=ctx), W_TILT), GAMMA, ctx=ctx)),
    # |x - shift(x)|: value 0 is read by the warp and again by the absdiff
    "absdiff_with_its_shifted_self": (lambda: Chain(Combine("absdiff", None, W_SHIFT)),
                                      lambda img, ctx: np.abs(img.astype(np.int16) - _warp(img, W_SHIFT)).astype(np.uint8)),
    "warp_first": (lambda: Chain([W_TILT_C, Invert()]), lambda img, ctx: 255 - _warp(img, W_TILT_C)),
    "warp_last": (lambda: Chain([Invert(), W_TILT_C]), lambda img, ctx: _warp(255 - img, W_TILT_C)),
    "two_warps": (lambda: Chain([FLIP_H, W_TILT]), lambda img, ctx: _warp(_warp(img, FLIP_H), W_TILT)),
    "table_warp_absdiff_with_value_0": (
        lambda: Chain.program([(Table(GAMMA), 0), (W_SHIFT, 1), ("absdiff", 0, 2)]),
        lambda img, ctx: np.abs(img.astype(np.int16) - _warp(GAMMA[img], W_SHIFT)).astype(np.uint8)),
}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_the_programs(vf_ctx, name):
    build, ref = PROGRAMS[name]
    c = build()
    assert any(st[0] == 12 for st in c.steps)
    wants = {}
    for shape in SHAPES:
        img = _frame(shape)
        keep = img.copy()
        want = wants[shape] = ref(img, vf_ctx)
        got = vfilter.chain(img, c, ctx=vf_ctx)
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)
        buf = img.copy()  # dst is src: the source is the staged copy
        assert vfilter.chain(buf, c, dst=buf, ctx=vf_ctx) is buf
        assert np.array_equal(buf, want), (name, shape, "in place")
    outs = vfilter.chain_frames([_frame(s) for s in SHAPES] + [np.empty((0, 0, 3), np.uint8)], c, ctx=vf_ctx)
    for s, o in zip(SHAPES, outs):
        assert np.array_equal(o, wants[s]), (name, s, "mixed")


def test_the_programs_are_what_they_are_chosen_for(vf_ctx):
    img = _frame(SHAPES[1])
    assert not np.array_equal(PROGRAMS["warp_first"][1](img, vf_ctx), PROGRAMS["warp_last"][1](img, vf_ctx))  # the order shows
    diff = PROGRAMS["absdiff_with_its_shifted_self"][1](img, vf_ctx)
    # the content moves 3 to the right and 2 up: dst(y, x) = src(y + 2, x - 3)
    assert np.array_equal(diff[:-2, 3:], np.abs(img[:-2, 3:].astype(np.int16) - img[2:, :-3]).astype(np.uint8))
    assert np.array_equal(diff[:, :3], img[:, :3]) and np.array_equal(diff[-2:], img[-2:])  # the border colour is 0: |x - 0|


def test_the_structured_forms_agree(vf_ctx):
    img = _frame(SHAPES[1])
    # a chain of one warp is the filter, and a Combine takes a Warp on either side
    assert np.array_equal(vfilter.chain(img, W_TILT, ctx=vf_ctx), vfilter.warp_affine(img, TILT, border="reflect101", ctx=vf_ctx))
    a = vfilter.chain(img, Combine("absdiff", W_SHIFT, None), ctx=vf_ctx)
    b = vfilter.chain(img, Combine("absdiff", None, W_SHIFT), ctx=vf_ctx)
    assert np.array_equal(a, b) and np.array_equal(a, PROGRAMS["absdiff_with_its_shifted_self"][1](img, vf_ctx))
    gray = img[:, :, 0].copy()  # one channel
    assert np.array_equal(vfilter.chain(gray, [Table(GAMMA), W_TILT, Invert()], ctx=vf_ctx), 255 - _warp(GAMMA[gray], W_TILT))
    mixed = vfilter.chain(img, [colors.gray(), FLIP_H], ctx=vf_ctx)
    assert np.array_equal(mixed, vfilter.transform(img, colors.gray(), ctx=vf_ctx)[:, ::-1])
