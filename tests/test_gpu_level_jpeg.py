"""The level filter on the JPEG path (``TurboJPEG.equalize_hist*``, ``auto_levels*``, ``filter_batch*`` with a
``Level``, chains with a level step, ``LevelWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_level_ref.py`` on the BGR frame, each frame by its own
histogram.  Whole JPEG byte strings are compared, nothing less.  The inputs are
``tests/test_gpu_sep_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4 and grayscale (decoded to three equal channels),
sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _chain_ref_level as CL
import _level_ref as L
from oracle import jpeg as J
from vfilter import Level, tables
from vfilter.filters import Chain, Invert
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (rule, mask, link, clips)
EQ = (L.EQUALIZE, 0, 0, (0, 0))
ST = (L.STRETCH, 0, 0, (655, 655))
ST_LINK = (L.STRETCH, 0, 1, (1311, 0))
EQ_G = (L.EQUALIZE, 2, 0, (0, 0))
FILTERS = {"equalize": EQ, "stretch1pc": ST}

# (input subsampling, width, height)
INPUTS = [(J.TJSAMP_422, 16, 8), (J.TJSAMP_422, 17, 13), (J.TJSAMP_422, 250, 130), (J.TJSAMP_420, 17, 13),
          (J.TJSAMP_444, 9, 9), (J.TJSAMP_GRAY, 33, 17)]
BIG = 2  # the 250 x 130 4:2:2 input


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    return [J.encode(J.synthetic_scene(90 + i, h, w), 90, J.TJPF_BGR, ss) for i, (ss, w, h) in enumerate(INPUTS)]


_want_cache = {}


def want(j, filt, quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    key = (j,) + tuple(filt) + (quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = L.level(J.decode(j, J.TJPF_BGR, flags), *filt)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def level_of(filt) -> Level:
    rule, mask, link, clips = filt
    chans = None if mask == 0 else tuple(c for c in range(3) if mask >> c & 1)
    if rule == L.EQUALIZE:
        return Level.equalize(chans, bool(link))
    return Level.stretch((clips[0] / 65536, clips[1] / 65536), chans, bool(link))


@pytest.mark.parametrize("fname", sorted(FILTERS))
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j, filt = jpegs[i], FILTERS[fname]
    assert tj.filter_batch([j], level_of(filt), jpeg_subsample=out_ss)[0] == want(j, filt, subsample=out_ss), (INPUTS[i], out_ss)


def test_mixed_batch_and_the_one_step_chain(tj, jpegs):
    got = tj.equalize_hist_batch(jpegs)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, EQ), INPUTS[i]
    assert tj.filter_batch(jpegs, Level.equalize()) == got
    assert tj.chain_batch(jpegs, [Level.equalize()]) == got  # tj.equalize_hist is the one-step tj.chain
    assert tj.equalize_hist_batch([]) == []
    got = tj.auto_levels_batch(jpegs, 0.01)
    assert got == [want(j, ST) for j in jpegs] == tj.filter_batch(jpegs, Level.stretch(0.01))
    j = jpegs[BIG]
    assert tj.equalize_hist(j) == want(j, EQ) == tj.chain(j, Chain(Level.equalize()))
    assert tj.auto_levels(j, (0.02, 0.0), link=True) == want(j, ST_LINK)
    assert tj.filter_batch([j], Level.equalize(channels=(1,)))[0] == want(j, EQ_G)
    assert len({want(j, EQ), want(j, ST), want(j, ST_LINK), want(j, EQ_G)}) == 4  # the filters differ in the bytes
    assert tj.equalize_hist(j, quality=60, jpeg_subsample=J.TJSAMP_420) == want(j, EQ, 60, J.TJSAMP_420)


def test_the_submit_and_wait_forms(tj, jpegs):
    t1 = tj.filter_batch_submit(jpegs, Level.equalize())
    t2 = tj.filter_batch_submit(jpegs, Level.stretch(0.01))
    t_raw = tj.ctx.jpeg_level_submit(jpegs, L.STRETCH, 0, 1, 1311, 0, 85, J.TJSAMP_422, 0)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, ST) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, EQ) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, ST_LINK) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]
    assert tj.ctx.jpeg_level(jpegs, L.EQUALIZE, 2, 0, 0, 0, 85, J.TJSAMP_422, 0) == [want(j, EQ_G) for j in jpegs]


def test_a_chain_with_a_level_step(tj, jpegs):
    """An equalisation into an inversion, between one decode and one encode; every frame by its own histogram."""
    prog = [("level", 0) + ST_LINK, ("table", 1, np.arange(255, -1, -1).astype(np.uint8))]
    got = tj.chain_batch(jpegs, Chain([level_of(ST_LINK), Invert()]))
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == J.encode(CL.run(J.decode(j, J.TJPF_BGR), prog), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]


def test_bad_filters_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.auto_levels(jpegs[0], 0.5)
    with pytest.raises(vfilter.VFilterError, match="unknown level rule 2"):
        tj.ctx.jpeg_level(jpegs, 2, 0, 0, 0, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="channel mask 8"):
        tj.ctx.jpeg_level_submit(jpegs, 0, 8, 0, 0, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="takes no clips"):
        tj.ctx.jpeg_level(jpegs, 0, 0, 0, 7, 0, 85, J.TJSAMP_422, 0)
    assert tj.equalize_hist(jpegs[0]) == want(jpegs[0], EQ)


def test_jpeg_bench_level_runs(tj, jpegs):
    ms, stages = tj.ctx.jpeg_bench_level([jpegs[BIG]] * 2, L.EQUALIZE, 0, 0, 0, 0, 85, J.TJSAMP_422, 0, iters=2)
    assert ms > 0 and isinstance(stages, dict)


def test_level_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.level_worker import LevelWorker, level_from_options
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = LevelWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, level=level_from_options(equalize=True), **kw)
    try:
        assert bytes(w(j)) == want(j, EQ)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, EQ), want(jpegs[0], EQ)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, EQ), want(jpegs[3], EQ)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, EQ) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], EQ)
    finally:
        w.close()
    rng = np.random.default_rng(63)
    frame = rng.integers(30, 200, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    w = LevelWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, level=level_from_options(stretch=[0.01]), **kw)
    try:
        assert bytes(w(frame.tobytes())) == L.level(frame, *ST).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        gray = rng.integers(0, 256, (12, 10), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == L.level(small, *ST).tobytes() and bytes(res[1]) == L.level(frame, *ST).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == L.level(frame, *ST).tobytes() and isinstance(bad[1], Exception)
        res = w.process_batch([gray.tobytes()], [wire.FrameMeta(0, 120, [12, 10])], [None])  # a 1-channel frame works
        assert bytes(res[0]) == L.level(gray, *ST).tobytes()
    finally:
        w.close()


def test_the_other_filters_are_unchanged_after_level_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.equalize_hist(j) == want(j, EQ)
    assert tj.invert_batch(jpegs) == [J.invert_jpeg(x) for x in jpegs]
    t = tables.gamma(2.2)
    assert tj.lut(j, t) == J.encode(t[J.decode(j, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.equalize_hist(j) == want(j, EQ)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a level filter
