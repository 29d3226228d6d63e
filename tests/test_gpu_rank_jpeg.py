"""The rank filters on the JPEG path (``TurboJPEG.erode*``, ``dilate*``, ``median_blur*``,
``RankWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_rank_ref.py`` on the BGR frame.  Whole JPEG byte
strings are compared, nothing less.  The filters are the 3 x 3 median and an erosion by the 3 wide
x 5 high rectangle (a transposed element fails); a dilation by a random 7 x 7 mask without its
centre covers the borders; the inputs cover 4:2:2, 4:2:0, 4:4:4 and grayscale, sizes that are not
whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _conv_ref as C
import _rank_ref as R
from oracle import jpeg as J
from vfilter import elements, tables
from vfilter.filters import Rank
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

ES = R.element_set()
MED3 = ("median", 3)
ER35 = ("erode", ES["rect3x5"])
DR7 = ("dilate", ES["random7"])
G3 = C.kernel_set()["gaussian3"]

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


def want(j, filt, border="constant", quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    op, arg = filt
    key = (j, op, np.asarray(arg).tobytes(), np.asarray(arg).shape, border, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = R.apply(J.decode(j, J.TJPF_BGR, flags), op, arg, border)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def rank_of(filt, border="constant"):
    op, arg = filt
    return Rank.median(arg) if op == "median" else Rank(op, arg, border)


def run(tj, j, filt, border="constant", **kw):
    op, arg = filt
    if op == "median":
        return tj.median_blur(j, arg, **kw)
    return (tj.erode if op == "erode" else tj.dilate)(j, arg, border=border, **kw)


@pytest.mark.parametrize("fname", ["median3", "erode3x5"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j = jpegs[i]
    filt = MED3 if fname == "median3" else ER35
    assert run(tj, j, filt, jpeg_subsample=out_ss) == want(j, filt, subsample=out_ss), (INPUTS[i], out_ss)


@pytest.mark.parametrize("border", ["reflect101", "replicate", "constant"])
def test_mixed_batch(tj, jpegs, border):
    got = tj.dilate_batch(jpegs, DR7[1], border=border)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, DR7, border), (INPUTS[i], border)
    assert tj.dilate_batch([], DR7[1]) == [] and tj.median_blur_batch([], 3) == []
    assert tj.erode_batch(jpegs, ER35[1], border=border) == [want(j, ER35, border) for j in jpegs]
    assert tj.median_blur_batch(jpegs, 5) == [want(j, ("median", 5)) for j in jpegs]


def test_turbojpeg_2_quality_and_the_identity_element(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).median_blur(j, 3) == want(j, MED3, tj_version=2)
    assert tj.median_blur(j, 3, quality=60) == want(j, MED3, quality=60)
    assert tj.erode(j) == want(j, ("erode", R.rect(3)))  # element=None: the 3 x 3 rectangle
    assert tj.dilate(j, elements.cross(5)) == want(j, ("dilate", R.cross(5)))
    assert tj.erode(j, elements.rect(7)) == want(j, ("erode", R.rect(7)))
    # the 1 x 1 element is the plain decode -> encode round trip
    plain = J.encode(J.decode(j, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.erode(j, np.ones((1, 1), np.uint8)) == plain and tj.dilate(j, [[1]]) == plain


def test_a_resynchronised_batch_is_filtered_once(tj, jpegs, monkeypatch):
    """With one queued span pass the decode checks report the sync unconverged at the wait; the
    remaining passes, every decode stage after them, the filter and the encode run again.  The
    result is the filter applied once: not twice (a second pass over filtered pixels), not zero
    times (the encoder reading the unfiltered buffer)."""
    monkeypatch.setenv("VF_JPEG_SYNC", "pass")
    monkeypatch.setenv("VF_JPEG_SYNC_G", "4")
    monkeypatch.setenv("VF_JPEG_SYNC_QUEUED", "1")
    noise = np.random.default_rng(81).integers(0, 256, (512, 640, 3), dtype=np.uint8)
    wide = J.encode(noise, 90, J.TJPF_BGR, J.TJSAMP_420)
    assert len(wide) > 4 * 256 * 4 * 32
    batch = [jpegs[BIG], wide]
    wants = [want(j, ER35) for j in batch]
    assert tj.erode_batch(batch, ER35[1]) == wants
    assert tj.erode(jpegs[BIG], ER35[1]) == wants[0]
    assert [bytes(v) for v in tj.invert_batch_result(tj.filter_batch_submit(batch, rank_of(ER35)))] == wants
    once = R.erode(J.decode(wide, J.TJPF_BGR), ER35[1])
    twice = J.encode(R.erode(once, ER35[1]), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert wants[1] != twice and wants[1] != J.encode(J.decode(wide, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_three_batches_in_flight_keep_their_own_filters(tj, jpegs):
    e = np.array(DR7[1], dtype=np.uint8)
    r = Rank.dilate(e, "replicate")
    t1 = tj.filter_batch_submit(jpegs, r)
    e[:] = 0  # the element was copied when the Rank was built ...
    raw = np.array(ER35[1], dtype=np.uint8)
    t_raw = tj.ctx.jpeg_rank_submit(jpegs, 0, raw, 2, 85, J.TJSAMP_422, 0)
    raw[:] = 0  # ... and again by the library at submit: this array went straight to the C call
    t2 = tj.filter2d_batch_submit(jpegs, G3)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == \
        [J.encode(C.filter2d(J.decode(j, J.TJPF_BGR), *G3), 85, J.TJPF_BGR, J.TJSAMP_422) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, DR7, "replicate") for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, ER35) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_filters_are_refused(tj, jpegs):
    with pytest.raises(ValueError):
        tj.erode(jpegs[0], np.ones((2, 2)))
    with pytest.raises(ValueError):
        tj.median_blur(jpegs[0], 7)
    with pytest.raises(ValueError):
        tj.dilate_batch(jpegs, None, border="wrap")
    with pytest.raises(ValueError):
        tj.filter_batch_submit(jpegs, Rank.erode(np.zeros((3, 3))))
    assert tj.median_blur(jpegs[0], 3) == want(jpegs[0], MED3)


def test_rank_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.rank_worker import RankWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = RankWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, rank=Rank.median(3), **kw)
    try:
        assert bytes(w(j)) == want(j, MED3)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, MED3), want(jpegs[0], MED3)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, MED3), want(jpegs[3], MED3)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, MED3) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], MED3)
    finally:
        w.close()
    rng = np.random.default_rng(62)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    e35 = ER35[1]
    w = RankWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, rank=Rank.erode(e35, "replicate"), **kw)
    try:
        assert bytes(w(frame.tobytes())) == R.erode(frame, e35, "replicate").tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == R.erode(small, e35, "replicate").tobytes()
        assert bytes(res[1]) == R.erode(frame, e35, "replicate").tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == R.erode(frame, e35, "replicate").tobytes() and isinstance(bad[1], Exception)
    finally:
        w.close()
    frames = [rng.integers(0, 256, (12, 10, 3), dtype=np.uint8) for _ in range(3)]
    w = RankWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, rank=Rank.median(5), shape=(12, 10, 3), **kw)
    try:
        assert bytes(w(frames[0].tobytes())) == R.median(frames[0], 5).tobytes()
        out1 = np.empty(360, np.uint8)
        res = w.process_batch([f.tobytes() for f in frames], [None] * 3, [None, out1, None])
        assert res[1] is out1
        assert [bytes(r) for r in res] == [R.median(f, 5).tobytes() for f in frames]
        h = w.submit_batch([f.tobytes() for f in frames], [None] * 3, [None] * 3)
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [R.median(f, 5).tobytes() for f in frames]
    finally:
        w.close()
    with pytest.raises(ValueError):
        RankWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, rank="median", **kw)


def test_the_other_filters_are_unchanged_after_rank_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.median_blur(j, 3) == want(j, MED3)
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert tj.erode(j, ER35[1]) == want(j, ER35)
    t = tables.gamma(2.2)
    for x in jpegs:
        assert tj.lut(x, t) == J.encode(t[J.decode(x, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.median_blur(j, 3) == want(j, MED3)
    assert tj.filter2d(j, G3) == J.encode(C.filter2d(J.decode(j, J.TJPF_BGR), *G3), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.median_blur(j, 3) == want(j, MED3)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a rank filter
    img = J.decode(j, J.TJPF_BGR)
    assert tj.encode(img) == J.encode(img, 85, J.TJPF_BGR, J.TJSAMP_422)  # an encode too: it reads d_pix_ again
