"""Filter chains that hold a colour-matrix step against the interpreter of ``tests/_chain_ref_mix.py``
(``tests/_chain_ref.py``'s plus the ``mix`` step), bit for bit: hand-written programs -- ``edges`` on a
picture taken to gray first, a blur into sepia, ``absdiff(gray x, x)``, two matrices in sequence, a
matrix whose operand is read again later (it may not run in place) -- and 32 seeded random programs
that each hold at least one mix step, on 3 x 2 x 3 and 17 x 13 x 3 (W x H x C).  Eight of the random
programs also run on a 1366 x 520 x 3 frame in 1 MiB of staging: three bands.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_mix as CM
import _conv_ref
import _mix_ref as M
import _rank_ref as R
import vfilter
from vfilter import Mix
from vfilter.filters import Chain, Kernel, Rank, Table

pytestmark = pytest.mark.gpu

GRAY = ("mix", M.mat([[3735, 19235, 9798]] * 3), 15, "half_up")
SEPIA = ("mix", M.mat([[34, 137, 70], [43, 176, 89], [48, 197, 101]]), 8, "half_even")


def _mix(step, a):
    return (step[0], a) + step[1:]


def hand_written():
    el = R.element_set()
    g3 = _conv_ref.kernel_set()["gaussian3"]
    return {
        # gray -> median3 -> gradient rect3 -> threshold
        "gray_edges": [_mix(GRAY, 0), ("rank", 1, "median", 3, "replicate"), ("rank", 2, "dilate", el["rect3"], "constant"),
                       ("rank", 2, "erode", el["rect3"], "constant"), ("bin", "subtract", 3, 4),
                       ("table", 5, CR.threshold_table())],
        "blur_sepia": [("conv", 0, g3[0], g3[1], "reflect101"), _mix(SEPIA, 1)],
        "absdiff_gray": [_mix(GRAY, 0), ("bin", "absdiff", 1, 0)],
        "mix_mix": [_mix(SEPIA, 0), _mix(GRAY, 1)],
        # value 1 is read by the mix and again by the max: the mix may not overwrite it
        "operand_read_later": [("conv", 0, g3[0], g3[1], "replicate"), _mix(SEPIA, 1), ("bin", "max", 2, 1)],
        "table_mix_table": [("table", 0, CR.INVERT), _mix(SEPIA, 1), ("table", 2, CR.curves_table())],
    }


def to_chain(prog) -> Chain:
    entries = []
    for st in prog:
        if st[0] == "mix":
            entries.append((Mix((np.asarray(st[2]), st[3]), st[4]), st[1]))
        elif st[0] == "table":
            entries.append((Table(np.asarray(st[2])), st[1]))
        elif st[0] == "conv":
            entries.append((Kernel((np.asarray(st[2]), st[3]), st[4]), st[1]))
        elif st[0] == "rank":
            entries.append((Rank.median(st[3]) if st[2] == "median" else Rank(st[2], st[3], st[4]), st[1]))
        else:
            entries.append((st[1], st[2], st[3]))
    return Chain.program(entries)


HAND = hand_written()
RANDOM = CM.programs(32)
# (h, w, c)
SHAPES = [(2, 3, 3), (13, 17, 3)]
HAND_SHAPES = SHAPES + [(40, 175, 3)]
_FRAMES = {s: CR.noise(*s) for s in HAND_SHAPES}
_WANT = {}


def _want(name, shape):
    """The reference's result, computed once and shared (never written to)."""
    if (name, shape) not in _WANT:
        out = CM.run(_FRAMES[shape], (HAND if name in HAND else RANDOM)[name])
        out.flags.writeable = False
        _WANT[(name, shape)] = out
    return _WANT[(name, shape)]


def test_the_programs_are_what_they_are_chosen_for():
    assert len(RANDOM) == 32 and all(any(st[0] == "mix" for st in p) for p in RANDOM.values())
    assert sum(1 for p in RANDOM.values() if sum(st[0] == "mix" for st in p) >= 2) > 0
    assert {st[4] for p in RANDOM.values() for st in p if st[0] == "mix"} == set(CM.ROUNDINGS)
    assert any(st[0] == "mix" and st[3] == 0 for p in RANDOM.values() for st in p)
    big = _FRAMES[(40, 175, 3)]
    for name in HAND:
        out = _want(name, (40, 175, 3))
        assert out.any() and len(np.unique(out)) > 1 and not np.array_equal(out, big), name
    g = CM.run(big, HAND["absdiff_gray"][:1])
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_hand_written_programs(vf_ctx, name):
    c = to_chain(HAND[name])
    assert c.has_mix
    for shape in HAND_SHAPES:
        img = _FRAMES[shape]
        keep = img.copy()
        got = vfilter.chain(img, c, ctx=vf_ctx)
        want = _want(name, shape)
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)
        buf = img.copy()  # dst is src
        assert vfilter.chain(buf, c, dst=buf, ctx=vf_ctx) is buf
        assert np.array_equal(buf, want), (name, shape, "in place")
    outs = vfilter.chain_frames([_FRAMES[s] for s in HAND_SHAPES], c, ctx=vf_ctx)
    for s, o in zip(HAND_SHAPES, outs):
        assert np.array_equal(o, _want(name, s)), (name, s, "mixed")


def test_the_structured_forms_agree(vf_ctx):
    from vfilter import colors
    from vfilter.filters import Combine, Morph
    img = _FRAMES[(40, 175, 3)]
    edges = Chain([colors.gray(), Rank.median(3), Morph("gradient"), Table(CR.threshold_table())])
    assert np.array_equal(vfilter.chain(img, edges, ctx=vf_ctx), _want("gray_edges", (40, 175, 3)))
    ad = Chain([Combine("absdiff", colors.gray(), None)])
    assert np.array_equal(vfilter.chain(img, ad, ctx=vf_ctx), _want("absdiff_gray", (40, 175, 3)))
    one = vfilter.chain(img, [Mix(colors.sepia())], ctx=vf_ctx)  # a one-step chain is the single filter
    assert np.array_equal(one, vfilter.transform(img, colors.sepia(), ctx=vf_ctx))
    assert np.array_equal(one, M.mix(img, SEPIA[1], 8))


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_every_random_program_on_every_frame(vf_ctx, name):
    c = to_chain(RANDOM[name])
    for shape in SHAPES:
        img = _FRAMES[shape]
        keep = img.copy()
        got = vfilter.chain(img, c, ctx=vf_ctx)
        want = _want(name, shape)
        assert got.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)
    outs = vfilter.chain_frames([_FRAMES[s] for s in SHAPES], c, ctx=vf_ctx)
    for s, o in zip(SHAPES, outs):
        assert np.array_equal(o, _want(name, s)), (name, s, "mixed")


# ---- bands ------------------------------------------------------------------------------------------

CAP = 1 << 20
BAND_SHAPE = (520, 1366, 3)  # rows of 4098 bytes: 255 fit the staging


def _bands(W, H, C, ry, capacity):
    """``vf::conv::bands`` (csrc/vf_conv_bands.h): (y0, y1, s0, s1) per band."""
    rows = min(capacity // (W * C), H)
    out, y0 = [], 0
    while y0 < H:
        s0 = max(y0 - ry, 0)
        y1 = H if s0 + rows >= H else s0 + rows - ry
        assert y1 > y0
        out.append((y0, y1, s0, min(y1 + ry, H)))
        y0 = y1
    return out


# the eight cheapest for the reference among those with a vertical reach: a band then has a halo
BAND_NAMES = sorted((n for n in RANDOM if CM.reach(RANDOM[n]) >= 1), key=lambda n: (CM.cost(RANDOM[n]), n))[:8]


def test_the_band_cases_are_three_bands():
    h, w, c = BAND_SHAPE
    assert len(BAND_NAMES) == 8
    for name in BAND_NAMES:
        assert len(_bands(w, h, c, CM.reach(RANDOM[name]), CAP)) == 3, name


@pytest.mark.parametrize("name", BAND_NAMES)
def test_eight_random_programs_in_three_bands(name):
    big = CR.noise(*BAND_SHAPE, seed=11)
    want = CM.run(big, RANDOM[name])
    c = to_chain(RANDOM[name])
    with vfilter.Context(0, max_frame_bytes=CAP, max_batch=1) as ctx:
        got = vfilter.chain(big, c, ctx=ctx)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        buf = big.copy()  # dst is src: a band's halo rows are the band before's output
        assert vfilter.chain(buf, c, dst=buf, ctx=ctx) is buf
        assert np.array_equal(buf, want), (name, "in place", np.argwhere(buf != want)[:5])


def test_a_chain_with_a_mix_on_one_channel_frames_raises(vf_ctx):
    c = to_chain(HAND["gray_edges"])
    gray = np.ascontiguousarray(_FRAMES[(13, 17, 3)][..., 0])
    with pytest.raises(ValueError, match="colour matrix"):
        vfilter.chain(gray, c, ctx=vf_ctx)
    with pytest.raises(ValueError, match="colour matrix"):
        vfilter.chain_frames([gray[..., None].copy()], c, ctx=vf_ctx)
    # and by the library itself
    with pytest.raises(vfilter.VFilterError, match="a colour matrix on 1-channel frames"):
        vf_ctx.chain_frames_host([gray], [np.empty_like(gray)], [17], [13], 1, *c.args)
    assert np.array_equal(vfilter.chain(_FRAMES[(13, 17, 3)], c, ctx=vf_ctx), _want("gray_edges", (13, 17, 3)))
