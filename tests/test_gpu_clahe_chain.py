"""Filter chains that hold a CLAHE step against the interpreter of ``tests/_chain_ref_clahe.py``, bit for bit,
on 13 x 17 and 130 x 250 frames (W x H): a luma-only CLAHE through two colour matrices, a ``Combine`` that
reads the CLAHE step's operand twice (so the step may not run in place), two CLAHE steps with different
grids in one program (two sets of scratch), a table before and after (nothing folds across), and a level
step beside a CLAHE step.  Every program runs out of place, in place and in a mixed batch.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_clahe as CC
import _level_ref as L
import _mix_ref as M
import vfilter
from vfilter import Clahe, Level, Mix
from vfilter.filters import Chain, Combine, Invert, Table

pytestmark = pytest.mark.gpu

TO_YCC = ("mix", M.mat([[29, 150, 77], [128, -85, -43], [-21, -107, 128]], (0, 128 << 8, 128 << 8)), 8, "half_even")
FROM_YCC = ("mix", M.mat([[256, 454, 0], [256, -88, -183], [256, 0, 359]], (-454 * 128, (88 + 183) * 128, -359 * 128)), 8,
            "half_even")
GAMMA = CR.gamma_table(0.7)
INVERT = np.arange(255, -1, -1).astype(np.uint8)

HAND = {
    "luma_only": [(TO_YCC[0], 0) + TO_YCC[1:], ("clahe", 1, 512, 8, 8, 1), (FROM_YCC[0], 2) + FROM_YCC[1:]],
    # max(x, clahe(x)): value 0 is read again, so the CLAHE step may not run in place
    "combine_reads_the_operand_twice": [("clahe", 0, 512, 4, 2, 0), ("bin", "max", 0, 1)],
    "two_clahe_steps": [("clahe", 0, 1024, 8, 8, 0), ("clahe", 1, 256, 3, 5, 5)],
    "table_before_and_after": [("table", 0, GAMMA), ("clahe", 1, 512, 8, 8, 0), ("table", 2, INVERT)],
    "level_then_clahe": [("level", 0, L.STRETCH, 0, 1, (655, 655)), ("clahe", 1, 640, 2, 16, 0)],
}


def to_chain(prog) -> Chain:
    entries = []
    for st in prog:
        if st[0] == "clahe":
            q, tx, ty, mask = st[2:]
            f = Clahe(q / 256, (tx, ty), None if mask == 0 else tuple(c for c in range(3) if mask >> c & 1))
            assert f.args == (q, tx, ty, mask)
            entries.append((f, st[1]))
        elif st[0] == "level":
            rule, mask, link, clips = st[2:]
            assert rule == L.STRETCH and mask == 0
            entries.append((Level.stretch((clips[0] / 65536, clips[1] / 65536), None, bool(link)), st[1]))
        elif st[0] == "mix":
            entries.append((Mix((np.asarray(st[2]), st[3]), st[4]), st[1]))
        elif st[0] == "table":
            entries.append((Table(np.asarray(st[2])), st[1]))
        else:
            entries.append((st[1], st[2], st[3]))
    return Chain.program(entries)


SHAPES = [(17, 13, 3), (250, 130, 3)]  # (h, w, c)
_FRAMES = {s: (CR.noise(*s) // 2 + 40) for s in SHAPES}  # a narrow range: the filter has work to do
_WANT = {}


def _want(name, shape):
    """The reference's result, computed once and shared (never written to)."""
    if (name, shape) not in _WANT:
        out = CC.run(_FRAMES[shape], HAND[name])
        out.flags.writeable = False
        _WANT[(name, shape)] = out
    return _WANT[(name, shape)]


def test_the_programs_are_what_they_are_chosen_for():
    big = _FRAMES[(250, 130, 3)]
    for name in HAND:
        out = _want(name, (250, 130, 3))
        assert len(np.unique(out)) > 8 and not np.array_equal(out, big), name
    through = CC.run(big, [HAND["luma_only"][0], (FROM_YCC[0], 1) + FROM_YCC[1:]])
    assert not np.array_equal(_want("luma_only", (250, 130, 3)), through)  # the step between the matrices does something
    one = CC.run(big, HAND["two_clahe_steps"][:1])
    assert not np.array_equal(_want("two_clahe_steps", (250, 130, 3)), one)


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
    luma = Chain([Mix((np.asarray(TO_YCC[1]), 8)), Clahe(2.0, channels=[0]), Mix((np.asarray(FROM_YCC[1]), 8))])
    assert np.array_equal(vfilter.chain(img, luma, ctx=vf_ctx), _want("luma_only", shape))
    comb = Chain(Combine("max", None, Clahe(2.0, (4, 2))))
    assert np.array_equal(vfilter.chain(img, comb, ctx=vf_ctx), _want("combine_reads_the_operand_twice", shape))
    assert np.array_equal(vfilter.chain(img, [Table(GAMMA), Clahe(2.0), Invert()], ctx=vf_ctx),
                          _want("table_before_and_after", shape))
    # a chain of one CLAHE step is the filter
    assert np.array_equal(vfilter.chain(img, Clahe(2.0), ctx=vf_ctx), vfilter.clahe(img, 2.0, ctx=vf_ctx))
    gray = img[:, :, 0].copy()  # one channel
    assert np.array_equal(vfilter.chain(gray, [Table(GAMMA), Clahe(2.0), Invert()], ctx=vf_ctx),
                          CC.run(gray, HAND["table_before_and_after"]))
