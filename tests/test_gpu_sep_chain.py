"""Filter chains that hold a separable step against the interpreter of ``tests/_chain_ref_sep.py``
(``tests/_chain_ref.py``'s plus the ``sep`` step), bit for bit: hand-written programs -- a blur into a
threshold, an unsharp mask built from a 15 x 15 mean, gray -> Gaussian -> gradient, two separable
steps in a row with a vertical reach of 30 rows, a separable step whose operand is read again
later -- and 32 seeded random programs that each hold at least one sep step, on 3 x 2 x 3 and
40 x 33 x 3 (W x H x C).  Eight of the random programs also run on a 1366 x 520 x 3 frame in 1 MiB of
staging: three bands.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_mix as CM
import _chain_ref_sep as CS
import _mix_ref as M
import _rank_ref as RR
import _sep_ref as S
import vfilter
from vfilter import Mix, Separable
from vfilter import kernels as K
from vfilter.filters import Chain, Combine, Kernel, Morph, Rank, Table

pytestmark = pytest.mark.gpu

GRAY = ("mix", M.mat([[3735, 19235, 9798]] * 3), 15, "half_up")
G15 = np.array([1, 2, 6, 11, 20, 30, 38, 40, 38, 30, 20, 11, 6, 2, 1])  # gaussian_taps(15, 2.5): sums to 256
ONES = lambda n: np.ones(n, np.int64)  # noqa: E731
_R31X, _R31Y, _R31S = S.kernel_set()["rand31x31"]


def _run(img, prog):
    """``_chain_ref_sep.run`` with the colour-matrix step of ``_chain_ref_mix`` as well."""
    vals = [np.asarray(img)]
    for st in prog:
        if st[0] == "mix":
            vals.append(M.mix(vals[st[1]], st[2], st[3], st[4]))
        elif st[0] == "bin":
            vals.append(CR.binary(st[1], vals[st[2]], vals[st[3]]))
        else:
            vals.append(CS.run(vals[st[1]], [(st[0], 0) + tuple(st[2:])]))
    return vals[-1]


def hand_written():
    el = RR.element_set()
    return {
        "blur_threshold": [("sep", 0, ONES(5), ONES(5), 0, 25, "half_even", "reflect101"), ("table", 1, CR.threshold_table(128))],
        # x + (x - mean15(x)), both saturating: value 0 is read three times
        "unsharp15": [("sep", 0, ONES(15), ONES(15), 0, 225, "half_even", "reflect101"), ("bin", "subtract", 0, 1),
                      ("bin", "add", 0, 2)],
        "gray_gaussian_gradient": [(GRAY[0], 0) + GRAY[1:], ("sep", 1, G15, G15, 16, 1, "half_up", "reflect101"),
                                   ("rank", 2, "dilate", el["rect3"], "constant"), ("rank", 2, "erode", el["rect3"], "constant"),
                                   ("bin", "subtract", 3, 4)],
        # reach 15 + 15 = 30 rows
        "sep_sep": [("sep", 0, _R31X, _R31Y, _R31S, 1, "half_even", "replicate"),
                    ("sep", 1, ONES(3), ONES(31), 0, 93, "half_even", "reflect101")],
        # value 1 is read by the sep and again by the max: the sep writes another buffer anyway
        "operand_read_later": [("table", 0, CR.gamma_table(0.7)), ("sep", 1, ONES(9), ONES(3), 0, 27, "half_even", "constant"),
                               ("bin", "max", 2, 1)],
        "rank_sep_table": [("rank", 0, "median", 3, "replicate"), ("sep", 1, G15, ONES(1), 8, 1, "half_even", "replicate"),
                           ("table", 2, CR.curves_table())],
    }


def to_chain(prog) -> Chain:
    entries = []
    for st in prog:
        if st[0] == "sep":
            kx, ky, shift, divisor, rounding, border = st[2:]
            entries.append((Separable((np.asarray(kx), 0), (np.asarray(ky), 0), shift, divisor, rounding, border), st[1]))
        elif st[0] == "mix":
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
RANDOM = CS.programs(32)
SHAPES = [(2, 3, 3), (33, 40, 3)]  # (h, w, c)
HAND_SHAPES = SHAPES + [(70, 175, 3)]
_FRAMES = {s: CR.noise(*s) for s in HAND_SHAPES}
_WANT = {}


def _want(name, shape):
    """The reference's result, computed once and shared (never written to)."""
    if (name, shape) not in _WANT:
        out = _run(_FRAMES[shape], (HAND if name in HAND else RANDOM)[name])
        out.flags.writeable = False
        _WANT[(name, shape)] = out
    return _WANT[(name, shape)]


def test_the_programs_are_what_they_are_chosen_for():
    assert len(RANDOM) == 32 and all(any(st[0] == "sep" for st in p) for p in RANDOM.values())
    seps = [st for p in RANDOM.values() for st in p if st[0] == "sep"]
    assert any(st[5] > 1 for st in seps) and any(st[4] > 0 for st in seps)          # divisors and shifts
    assert {st[6] for st in seps if st[4] > 0} == set(CS.ROUNDINGS) and {st[7] for st in seps} == set(CS.BORDERS)
    assert max(len(st[3]) for st in seps) > 15 and max(len(st[2]) for st in seps) > 15
    assert CS.reach(HAND["sep_sep"]) == 30
    big = _FRAMES[(70, 175, 3)]
    for name in HAND:
        out = _want(name, (70, 175, 3))
        assert out.any() and len(np.unique(out)) > 1 and not np.array_equal(out, big), name


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_hand_written_programs(vf_ctx, name):
    c = to_chain(HAND[name])
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
    shape = (70, 175, 3)
    img = _FRAMES[shape]
    bt = Chain([Separable.box(5), Table(CR.threshold_table(128))])
    assert np.array_equal(vfilter.chain(img, bt, ctx=vf_ctx), _want("blur_threshold", shape))
    unsharp = Chain(Combine("add", None, Combine("subtract", None, Separable.box(15))))
    assert np.array_equal(vfilter.chain(img, unsharp, ctx=vf_ctx), _want("unsharp15", shape))
    assert K.gaussian_taps(15, 2.5)[0].tolist() == G15.tolist()
    ggg = Chain([colors.gray(), Separable.gaussian(15, 2.5), Morph("gradient")])
    assert np.array_equal(vfilter.chain(img, ggg, ctx=vf_ctx), _want("gray_gaussian_gradient", shape))
    one = vfilter.chain(img, [Separable.box((9, 3))], ctx=vf_ctx)  # a one-step chain is the single filter
    assert np.array_equal(one, vfilter.blur(img, (9, 3), ctx=vf_ctx)) and np.array_equal(one, S.box(img, 9, 3))
    gray = np.ascontiguousarray(img[..., 1])  # a chain of separable steps takes 1-channel frames too
    assert np.array_equal(vfilter.chain(gray, bt, ctx=vf_ctx), _run(gray, HAND["blur_threshold"]))


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
BAND_NAMES = sorted((n for n in RANDOM if CS.reach(RANDOM[n]) >= 1), key=lambda n: (CS.cost(RANDOM[n]), n))[:8]


def test_the_band_cases_are_three_bands():
    h, w, c = BAND_SHAPE
    assert len(BAND_NAMES) == 8
    for name in BAND_NAMES:
        assert len(_bands(w, h, c, CS.reach(RANDOM[name]), CAP)) == 3, name


@pytest.mark.parametrize("name", BAND_NAMES)
def test_eight_random_programs_in_three_bands(name):
    big = CR.noise(*BAND_SHAPE, seed=11)
    want = CS.run(big, RANDOM[name])
    c = to_chain(RANDOM[name])
    with vfilter.Context(0, max_frame_bytes=CAP, max_batch=1) as ctx:
        got = vfilter.chain(big, c, ctx=ctx)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        buf = big.copy()  # dst is src: a band's halo rows are the band before's output
        assert vfilter.chain(buf, c, dst=buf, ctx=ctx) is buf
        assert np.array_equal(buf, want), (name, "in place", np.argwhere(buf != want)[:5])


def test_the_reach_of_two_31_tap_steps_in_bands():
    """sep_sep has a reach of 30 rows: in 1 MiB of staging the 520-row frame is three bands, each
    uploaded with 30 rows of halo on either side."""
    h, w, c = BAND_SHAPE
    assert len(_bands(w, h, c, 30, CAP)) == 3
    big = CR.noise(*BAND_SHAPE, seed=12)
    want = _run(big, HAND["sep_sep"])
    with vfilter.Context(0, max_frame_bytes=CAP, max_batch=1) as ctx:
        got = vfilter.chain(big, to_chain(HAND["sep_sep"]), ctx=ctx)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
