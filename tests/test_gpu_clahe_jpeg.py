"""CLAHE on the JPEG path (``TurboJPEG.clahe*``, ``filter_batch*`` with a ``Clahe``, chains with a CLAHE step,
``ClaheWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_clahe_ref.py`` on the BGR frame.  Whole JPEG byte strings are
compared, nothing less.  The inputs are ``tests/test_gpu_level_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4 and grayscale
(decoded to three equal channels), sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _chain_ref_clahe as CC
import _clahe_ref as R
import _level_ref as L
from oracle import jpeg as J
from vfilter import Clahe, tables
from vfilter.filters import Chain, Invert
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (clip_q8, tiles_x, tiles_y, mask)
C2 = (512, 8, 8, 0)
C40 = (10240, 8, 8, 0)
C_GRID = (640, 4, 2, 0)
C_G = (512, 8, 8, 2)
FILTERS = {"limit2": C2, "limit2_5_grid_4x2": C_GRID}

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
        img = R.clahe(J.decode(j, J.TJPF_BGR, flags), *filt)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def clahe_of(filt) -> Clahe:
    q, tx, ty, mask = filt
    f = Clahe(q / 256, (tx, ty), None if mask == 0 else tuple(c for c in range(3) if mask >> c & 1))
    assert f.args == tuple(filt)
    return f


@pytest.mark.parametrize("fname", sorted(FILTERS))
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j, filt = jpegs[i], FILTERS[fname]
    assert tj.filter_batch([j], clahe_of(filt), jpeg_subsample=out_ss)[0] == want(j, filt, subsample=out_ss), (INPUTS[i], out_ss)


def test_mixed_batch_and_the_one_step_chain(tj, jpegs):
    got = tj.clahe_batch(jpegs, 2.0)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, C2), INPUTS[i]
    assert tj.filter_batch(jpegs, Clahe(2.0)) == got
    assert tj.chain_batch(jpegs, [Clahe(2.0)]) == got  # tj.clahe is the one-step tj.chain
    assert tj.clahe_batch([]) == []
    assert tj.clahe_batch(jpegs) == [want(j, C40) for j in jpegs]  # cv2's defaults
    j = jpegs[BIG]
    assert tj.clahe(j, 2.0) == want(j, C2) == tj.chain(j, Chain(Clahe(2.0)))
    assert tj.clahe(j, 2.5, (4, 2)) == want(j, C_GRID)
    assert tj.clahe(j, 2.0, channels=(1,)) == want(j, C_G)
    assert len({want(j, C2), want(j, C40), want(j, C_GRID), want(j, C_G)}) == 4  # the filters differ in the bytes
    assert tj.clahe(j, 2.0, quality=60, jpeg_subsample=J.TJSAMP_420) == want(j, C2, 60, J.TJSAMP_420)


def test_the_submit_and_wait_forms(tj, jpegs):
    t1 = tj.filter_batch_submit(jpegs, Clahe(2.0))
    t2 = tj.filter_batch_submit(jpegs, Clahe(2.5, (4, 2)))
    t_raw = tj.ctx.jpeg_clahe_submit(jpegs, 10240, 8, 8, 0, 85, J.TJSAMP_422, 0)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, C_GRID) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, C2) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, C40) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]
    assert tj.ctx.jpeg_clahe(jpegs, 512, 8, 8, 2, 85, J.TJSAMP_422, 0) == [want(j, C_G) for j in jpegs]


def test_a_chain_with_a_clahe_step(tj, jpegs):
    """CLAHE into an inversion, between one decode and one encode."""
    prog = [("clahe", 0) + C_GRID, ("table", 1, np.arange(255, -1, -1).astype(np.uint8))]
    got = tj.chain_batch(jpegs, Chain([clahe_of(C_GRID), Invert()]))
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == J.encode(CC.run(J.decode(j, J.TJPF_BGR), prog), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]


def test_bad_filters_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.clahe(jpegs[0], 0.3)
    with pytest.raises(vfilter.VFilterError, match="clip_q8=-1"):
        tj.ctx.jpeg_clahe(jpegs, -1, 8, 8, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="channel mask 8"):
        tj.ctx.jpeg_clahe_submit(jpegs, 512, 8, 8, 8, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="tiles_x=17"):
        tj.ctx.jpeg_clahe(jpegs, 512, 17, 8, 0, 85, J.TJSAMP_422, 0)
    assert tj.clahe(jpegs[0], 2.0) == want(jpegs[0], C2)


def test_jpeg_bench_clahe_runs(tj, jpegs):
    ms, stages = tj.ctx.jpeg_bench_clahe([jpegs[BIG]] * 2, 512, 8, 8, 0, 85, J.TJSAMP_422, 0, iters=2)
    assert ms > 0 and isinstance(stages, dict)


def test_clahe_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.clahe_worker import ClaheWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = ClaheWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, clahe=Clahe(2.0), **kw)
    try:
        assert bytes(w(j)) == want(j, C2)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, C2), want(jpegs[0], C2)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, C2), want(jpegs[3], C2)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, C2) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], C2)
    finally:
        w.close()
    rng = np.random.default_rng(63)
    frame = rng.integers(30, 200, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    w = ClaheWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, clahe=Clahe(2.5, (4, 2)), **kw)
    try:
        assert bytes(w(frame.tobytes())) == R.clahe(frame, *C_GRID).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        gray = rng.integers(0, 256, (12, 10), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == R.clahe(small, *C_GRID).tobytes() and bytes(res[1]) == R.clahe(frame, *C_GRID).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == R.clahe(frame, *C_GRID).tobytes() and isinstance(bad[1], Exception)
        res = w.process_batch([gray.tobytes()], [wire.FrameMeta(0, 120, [12, 10])], [None])  # a 1-channel frame works
        assert bytes(res[0]) == R.clahe(gray, *C_GRID).tobytes()
    finally:
        w.close()


def test_the_other_filters_are_unchanged_after_clahe_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.clahe(j, 2.0) == want(j, C2)
    assert tj.invert_batch(jpegs) == [J.invert_jpeg(x) for x in jpegs]
    t = tables.gamma(2.2)
    assert tj.lut(j, t) == J.encode(t[J.decode(j, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.equalize_hist(j) == J.encode(L.level(J.decode(j, J.TJPF_BGR), L.EQUALIZE), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.clahe(j, 2.0) == want(j, C2)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a CLAHE filter
