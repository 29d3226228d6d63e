"""Filter chains over the seeded random programs of ``tests/_chain_gen.py`` (64 generated and a few
hand-written ones per channel count: oblong kernels and elements, a border per step, ``a == b``,
shared and folding tables, in-place steps) against the numpy interpreter of ``tests/_chain_ref.py``.
Every comparison is exact.

The small frames, (h, w, c): 1 x 1 x 3, 2 x 3 x 3 (shorter than most reaches), 13 x 17 with one and
three channels, and 40 x 175 x 3: 525 row bytes and 40 rows are three 256-byte tiles by three 16-row
tiles, both edges partial.

The band test gives frames of 520 rows a staging of 1 MiB (the smallest a context takes), so a frame
of three bands cannot be much smaller than these.  4096 x 520 x 1 has rows of 4096 bytes, 256 fit;
1366 x 520 x 3 has rows of 4098 bytes, 255 fit.  A program of reach R gets output rows
[0, rows - R), [rows - R, 2 rows - 3R), [2 rows - 3R, 520) from source rows that start R above: with
R = 5 and 256 rows the bands end at rows 251, 497 and 520, with R = 3 and 255 rows at 252, 501 and
520, with R = 2 (``dog``) at 253, 504 and 520.  Every generated or hand-written program there has
two neighbourhood steps of different vertical radius reading one value, so on the interior band
the smaller one is handed a window that starts above ``lo - r``.  The programs are the cheapest of
the set that qualify: the numpy reference is the slow side of every case.

The JPEG test's reference is ``tests/test_gpu_chain_jpeg.py``'s: oracle decode, the interpreter,
oracle encode; whole JPEG byte strings are compared.
"""
import numpy as np
import pytest

import _chain_gen as G
import _chain_ref as CR
import vfilter
from _chain_build import to_chain

pytestmark = pytest.mark.gpu

NAMES = list(G.PROGRAMS)
assert NAMES == list(G.PROGRAMS_1)
# (h, w, c)
SHAPES = [(1, 1, 3), (2, 3, 3), (13, 17, 1), (13, 17, 3), (40, 175, 3)]
_FRAMES = {s: CR.noise(*s) for s in SHAPES}
_GRAY2 = np.ascontiguousarray(_FRAMES[(40, 175, 3)][:9, :21, 1])  # a second one-channel frame for the mixed call
_WANT = {}


def _prog(name, channels):
    return (G.PROGRAMS if channels == 3 else G.PROGRAMS_1)[name]


def _want(name, shape):
    """The reference's result, computed once and shared (never written to)."""
    if (name, shape) not in _WANT:
        out = CR.run(_FRAMES[shape], _prog(name, shape[2]))
        out.flags.writeable = False
        _WANT[(name, shape)] = out
    return _WANT[(name, shape)]


@pytest.mark.parametrize("name", NAMES)
def test_every_program_on_every_frame(vf_ctx, name):
    for shape in SHAPES:
        img = _FRAMES[shape]
        keep = img.copy()
        got = vfilter.chain(img, to_chain(_prog(name, shape[2])), ctx=vf_ctx)
        want = _want(name, shape)
        assert got.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, shape, np.argwhere(got != want)[:5])
        assert np.array_equal(img, keep)
    # once more, the frames of one channel count in one call of mixed sizes
    shapes = [s for s in SHAPES if s[2] == 3]
    outs = vfilter.chain_frames([_FRAMES[s] for s in shapes], to_chain(_prog(name, 3)), ctx=vf_ctx)
    for s, o in zip(shapes, outs):
        assert np.array_equal(o, _want(name, s)), (name, s, "mixed")
    gray = [_FRAMES[(13, 17, 1)], _GRAY2]
    outs = vfilter.chain_frames(gray, to_chain(_prog(name, 1)), ctx=vf_ctx)
    assert np.array_equal(outs[0], _want(name, (13, 17, 1))), (name, "mixed, one channel")
    assert np.array_equal(outs[1], CR.run(_GRAY2, _prog(name, 1))), (name, "mixed, one channel", _GRAY2.shape)


# ---- bands ------------------------------------------------------------------------------------------

def bands(W, H, C, ry, capacity):
    """``vf::conv::bands`` (csrc/vf_conv_bands.h): (y0, y1, s0, s1) per band."""
    row = W * C
    rows = min(capacity // row, H)
    out = []
    y0 = 0
    while y0 < H:
        s0 = max(y0 - ry, 0)
        y1 = H if s0 + rows >= H else s0 + rows - ry
        assert y1 > y0
        out.append((y0, y1, s0, min(y1 + ry, H)))
        y0 = y1
    return out


CAP = 1 << 20
# (h, w, c) of the banded frames
BAND_SHAPE = {1: (520, 4096, 1), 3: (520, 1366, 3)}
# (program, channels, also with dst is src)
BAND_CASES = [("g29", 3, True), ("g49", 3, False), ("x_subtract_over_b", 3, False),
              ("g02", 1, False), ("g26", 1, True), ("g53", 1, False), ("dog", 3, False), ("eight", 3, False)]
_BIG = {}


def _band_prog(name, channels):
    if name in ("dog", "eight"):
        return CR.program_set("reflect101", channels)[name]
    return _prog(name, channels)


def test_the_band_cases_are_what_they_are_chosen_for():
    for name, channels, _ in BAND_CASES:
        prog = _band_prog(name, channels)
        h, w, c = BAND_SHAPE[channels]
        R = CR.reach(prog)
        assert len(bands(w, h, c, R, CAP)) >= 3, (name, bands(w, h, c, R, CAP))
        assert sum(1 for st in prog if st[0] == "rank" and st[2] == "median" and st[3] == 5) <= 1, name
        if name not in ("dog", "eight"):
            assert 3 <= R <= 10 and "two_neighbourhood_readers_of_different_kh" in G.features(prog), name
    assert bands(4096, 520, 1, 5, CAP) == [(0, 251, 0, 256), (251, 497, 246, 502), (497, 520, 492, 520)]
    assert bands(1366, 520, 3, 3, CAP) == [(0, 252, 0, 255), (252, 501, 249, 504), (501, 520, 498, 520)]
    assert bands(1366, 520, 3, 2, CAP) == [(0, 253, 0, 255), (253, 504, 251, 506), (504, 520, 502, 520)]
    # the documented bands of tests/test_gpu_chain.py, by the same transcription
    assert [b[1] for b in bands(1024, 800, 3, 2, CAP)] == [339, 676, 800]
    assert [b[1] for b in bands(1024, 800, 3, 4, CAP)] == [337, 670, 800]


@pytest.mark.parametrize("name,channels,in_place", BAND_CASES)
def test_bands_of_a_frame_larger_than_the_staging(name, channels, in_place):
    if channels not in _BIG:
        _BIG[channels] = CR.noise(*BAND_SHAPE[channels], seed=7)
    big = _BIG[channels]
    prog = _band_prog(name, channels)
    want = CR.run(big, prog)
    c = to_chain(prog)

    def rows(got):
        bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
        return bad[:3], bad[-3:], bands(big.shape[1], big.shape[0], channels, CR.reach(prog), CAP)

    with vfilter.Context(0, max_frame_bytes=CAP, max_batch=1) as ctx:
        got = vfilter.chain(big, c, ctx=ctx)
        assert np.array_equal(got, want), (name, rows(got))
        if in_place:  # dst is src: a band's halo rows are the band before's output
            buf = big.copy()
            assert vfilter.chain(buf, c, dst=buf, ctx=ctx) is buf
            assert np.array_equal(buf, want), (name, "in place", rows(buf))


# ---- the JPEG path -----------------------------------------------------------------------------------

JPEG_NAMES = G.GENERATED[::5][:10] + sorted(n for n in NAMES if n.startswith("x_"))
assert len(JPEG_NAMES) == 16


@pytest.fixture(scope="module")
def tj(vf_ctx):
    from vfilter.jpeg import TurboJPEG
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    from oracle import jpeg as J
    # (width, height), both 4:2:2: neither is whole MCUs, the first is several kernel tiles wide
    return [J.encode(J.synthetic_scene(70 + i, h, w), 90, J.TJPF_BGR, J.TJSAMP_422) for i, (w, h) in enumerate([(175, 40), (17, 13)])]


def _jpeg_want(j, prog, subsample):
    from oracle import jpeg as J
    return J.encode(CR.run(J.decode(j, J.TJPF_BGR), prog), 85, J.TJPF_BGR, subsample)


@pytest.mark.parametrize("name", JPEG_NAMES)
def test_programs_on_the_jpeg_path(tj, jpegs, name):
    from oracle import jpeg as J
    prog = G.PROGRAMS[name]
    c = to_chain(prog)
    for i, j in enumerate(jpegs):
        assert tj.chain(j, c) == _jpeg_want(j, prog, J.TJSAMP_422), (name, i)
    assert tj.chain(jpegs[0], c, jpeg_subsample=J.TJSAMP_420) == _jpeg_want(jpegs[0], prog, J.TJSAMP_420), (name, "4:2:0")


def test_two_programs_in_flight_keep_their_own(tj, jpegs):
    from oracle import jpeg as J
    first, second = "x_subtract_over_b", "x_tables_fold"
    t1 = tj.chain_batch_submit(jpegs, to_chain(G.PROGRAMS[first]))
    t2 = tj.chain_batch_submit(jpegs, to_chain(G.PROGRAMS[second]))
    got2 = [bytes(v) for v in tj.invert_batch_result(t2)]
    got1 = [bytes(v) for v in tj.invert_batch_result(t1)]
    want1 = [_jpeg_want(j, G.PROGRAMS[first], J.TJSAMP_422) for j in jpegs]
    want2 = [_jpeg_want(j, G.PROGRAMS[second], J.TJSAMP_422) for j in jpegs]
    assert want1 != want2
    assert got1 == want1 and got2 == want2
