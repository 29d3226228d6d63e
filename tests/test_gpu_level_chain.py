"""Filter chains that hold a level step against the interpreter of ``tests/_chain_ref_level.py``
(``tests/_chain_ref.py``'s plus the ``level``, ``mix`` and ``sep`` steps), bit for bit, on 13 x 17 and
130 x 250 frames (W x H): a blur into an equalisation, a stretch into a sharpening, a ``Combine`` with a
``Level`` on one side, two level steps in one program, and a luma-only equalisation through two colour
matrices.  Every program runs out of place, in place and in a mixed batch.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_level as CL
import _level_ref as L
import _mix_ref as M
import vfilter
from vfilter import Level, Mix, Separable
from vfilter import kernels as K
from vfilter.filters import Chain, Combine, Kernel, Table

pytestmark = pytest.mark.gpu

ONES = lambda n: np.ones(n, np.int64)  # noqa: E731
SHARPEN = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]])
# BGR -> (luma, two chroma differences around 128) and roughly back, in 8-bit fixed point.  The pair is
# not an exact inverse and need not be: both sides of the comparison run the same integers.
TO_YCC = ("mix", M.mat([[29, 150, 77], [128, -85, -43], [-21, -107, 128]], (0, 128 << 8, 128 << 8)), 8, "half_even")
FROM_YCC = ("mix", M.mat([[256, 454, 0], [256, -88, -183], [256, 0, 359]], (-454 * 128, (88 + 183) * 128, -359 * 128)), 8,
            "half_even")


def hand_written():
    return {
        "box5_equalize": [("sep", 0, ONES(5), ONES(5), 0, 25, "half_even", "reflect101"), ("level", 1, L.EQUALIZE, 0, 0, (0, 0))],
        "stretch_sharpen": [("level", 0, L.STRETCH, 0, 0, (655, 655)), ("conv", 1, SHARPEN, 0, "reflect101")],
        # max(x, equalize(x)): value 0 is read again, so the level step may not run in place
        "combine_with_a_level": [("level", 0, L.EQUALIZE, 0, 1, (0, 0)), ("bin", "max", 0, 1)],
        "two_levels": [("level", 0, L.STRETCH, 0, 1, (1311, 66)), ("table", 1, CR.gamma_table(0.7)),
                       ("level", 2, L.EQUALIZE, 5, 0, (0, 0))],
        "luma_only": [(TO_YCC[0], 0) + TO_YCC[1:], ("level", 1, L.EQUALIZE, 1, 0, (0, 0)), (FROM_YCC[0], 2) + FROM_YCC[1:]],
    }


def to_chain(prog) -> Chain:
    entries = []
    for st in prog:
        if st[0] == "level":
            rule, mask, link, clips = st[2:]
            chans = None if mask == 0 else tuple(c for c in range(3) if mask >> c & 1)
            lv = Level.equalize(chans, bool(link)) if rule == L.EQUALIZE else \
                Level.stretch((clips[0] / 65536, clips[1] / 65536), chans, bool(link))
            assert (lv.clip_lo, lv.clip_hi) == tuple(clips)
            entries.append((lv, st[1]))
        elif st[0] == "sep":
            kx, ky, shift, divisor, rounding, border = st[2:]
            entries.append((Separable((np.asarray(kx), 0), (np.asarray(ky), 0), shift, divisor, rounding, border), st[1]))
        elif st[0] == "mix":
            entries.append((Mix((np.asarray(st[2]), st[3]), st[4]), st[1]))
        elif st[0] == "table":
            entries.append((Table(np.asarray(st[2])), st[1]))
        elif st[0] == "conv":
            entries.append((Kernel((np.asarray(st[2]), st[3]), st[4]), st[1]))
        else:
            entries.append((st[1], st[2], st[3]))
    return Chain.program(entries)


HAND = hand_written()
SHAPES = [(17, 13, 3), (250, 130, 3)]  # (h, w, c)
_FRAMES = {s: (CR.noise(*s) // 2 + 40) for s in SHAPES}  # a narrow range: both rules have work to do
_WANT = {}


def _want(name, shape):
    """The reference's result, computed once and shared (never written to)."""
    if (name, shape) not in _WANT:
        out = CL.run(_FRAMES[shape], HAND[name])
        out.flags.writeable = False
        _WANT[(name, shape)] = out
    return _WANT[(name, shape)]


def test_the_programs_are_what_they_are_chosen_for():
    big = _FRAMES[(250, 130, 3)]
    for name in HAND:
        out = _want(name, (250, 130, 3))
        assert len(np.unique(out)) > 8 and not np.array_equal(out, big), name
    luma = _want("luma_only", (250, 130, 3))
    through = CL.run(big, [HAND["luma_only"][0], (FROM_YCC[0], 1) + FROM_YCC[1:]])
    assert not np.array_equal(luma, through)  # the level step between the matrices does something
    assert K.sharpen()[0].tolist() == SHARPEN.tolist()


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_hand_written_programs(vf_ctx, name):
    c = to_chain(HAND[name])
    for shape in SHAPES:
        img = _FRAMES[shape]
        keep = img.copy()
        got = vfilter.chain(img, c, ctx=vf_ctx)
        want = _want(name, shape)
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)
        buf = img.copy()  # dst is src
        assert vfilter.chain(buf, c, dst=buf, ctx=vf_ctx) is buf
        assert np.array_equal(buf, want), (name, shape, "in place")
    outs = vfilter.chain_frames([_FRAMES[s] for s in SHAPES] + [np.empty((0, 0, 3), np.uint8)], c, ctx=vf_ctx)
    for s, o in zip(SHAPES, outs):
        assert np.array_equal(o, _want(name, s)), (name, s, "mixed")


def test_the_structured_forms_agree(vf_ctx):
    shape = (250, 130, 3)
    img = _FRAMES[shape]
    assert np.array_equal(vfilter.chain(img, [Separable.box(5), Level.equalize()], ctx=vf_ctx), _want("box5_equalize", shape))
    assert np.array_equal(vfilter.chain(img, [Level.stretch(0.01), Kernel(K.sharpen())], ctx=vf_ctx),
                          _want("stretch_sharpen", shape))
    comb = Chain(Combine("max", None, Level.equalize(link=True)))
    assert np.array_equal(vfilter.chain(img, comb, ctx=vf_ctx), _want("combine_with_a_level", shape))
    luma = Chain([Mix((np.asarray(TO_YCC[1]), 8)), Level.equalize(channels=(0,)), Mix((np.asarray(FROM_YCC[1]), 8))])
    assert np.array_equal(vfilter.chain(img, luma, ctx=vf_ctx), _want("luma_only", shape))
    # a chain of one level step is the level filter
    assert np.array_equal(vfilter.chain(img, Level.equalize(), ctx=vf_ctx), vfilter.equalize_hist(img, ctx=vf_ctx))
    gray = img[:, :, 0].copy()  # one channel: a level step needs none of the three
    assert np.array_equal(vfilter.chain(gray, [Level.stretch(0.01), Kernel(K.sharpen())], ctx=vf_ctx),
                          CL.run(gray, HAND["stretch_sharpen"]))
