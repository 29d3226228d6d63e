"""The convolution filter on the JPEG path (``TurboJPEG.filter2d*``, ``ConvWorker``) against the
oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_conv_ref.py`` on the BGR frame.  Whole JPEG byte
strings are compared, nothing less.  The kernels are the 3 x 3 Gaussian and a random 3 wide x 5
high kernel (a flipped or transposed kernel fails); the inputs cover 4:2:2, 4:2:0, 4:4:4 and
grayscale, sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _conv_ref as R
from oracle import jpeg as J
from vfilter import kernels as K
from vfilter import tables
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

KS = R.kernel_set()
G3 = KS["gaussian3"]
R35 = KS["random3x5"]

# (input subsampling, width, height)
INPUTS = [(J.TJSAMP_422, 16, 8), (J.TJSAMP_422, 17, 13), (J.TJSAMP_422, 250, 130), (J.TJSAMP_420, 17, 13),
          (J.TJSAMP_444, 9, 9), (J.TJSAMP_GRAY, 33, 17)]
BIG = 2  # the 250 x 130 4:2:2 input


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    return [J.encode(J.synthetic_scene(70 + i, h, w), 90, J.TJPF_BGR, ss) for i, (ss, w, h) in enumerate(INPUTS)]


_want_cache = {}


def want(j, kernel, border="reflect101", quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    w, s = kernel
    key = (j, np.asarray(w).tobytes(), np.asarray(w).shape, s, border, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = R.filter2d(J.decode(j, J.TJPF_BGR, flags), w, s, border)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


@pytest.mark.parametrize("kname", ["gaussian3", "random3x5"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, kname):
    j = jpegs[i]
    assert tj.filter2d(j, KS[kname], jpeg_subsample=out_ss) == want(j, KS[kname], subsample=out_ss), (INPUTS[i], out_ss)


@pytest.mark.parametrize("border", ["reflect101", "replicate", "constant"])
def test_mixed_batch(tj, jpegs, border):
    got = tj.filter2d_batch(jpegs, R35, border=border)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, R35, border), (INPUTS[i], border)
    assert tj.filter2d_batch([], G3) == []


def test_turbojpeg_2_quality_and_the_ready_made_kernels(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).filter2d(j, G3) == want(j, G3, tj_version=2)
    assert tj.filter2d(j, G3, quality=60) == want(j, G3, quality=60)
    assert tj.filter2d(j, K.gaussian3()) == want(j, G3)
    assert tj.filter2d(j, np.outer([1, 2, 1], [1, 2, 1]) / 16.0) == want(j, G3)  # a dyadic float kernel
    assert tj.filter2d(j, K.sharpen()) == want(j, KS["sharpen"])
    assert tj.filter2d(j, KS["random7"]) == want(j, KS["random7"])
    # the identity kernel is the plain decode -> encode round trip
    assert tj.filter2d(j, K.identity()) == J.encode(J.decode(j, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_a_resynchronised_batch_is_filtered_once(tj, jpegs, monkeypatch):
    """With one queued span pass the decode checks report the sync unconverged at the wait; the
    remaining passes, every decode stage after them, the filter and the encode run again.  The
    result is the filter applied once: not twice (a second pass over filtered pixels), not zero
    times (the encoder reading the unfiltered buffer)."""
    monkeypatch.setenv("VF_JPEG_SYNC", "pass")
    monkeypatch.setenv("VF_JPEG_SYNC_G", "4")
    monkeypatch.setenv("VF_JPEG_SYNC_QUEUED", "1")
    # noise: long enough for several span-sync workgroups (256 x G subsequences of 256 bits each), whose
    # exits pass 0 always changes, so one queued pass leaves the sync unconverged
    noise = np.random.default_rng(81).integers(0, 256, (512, 640, 3), dtype=np.uint8)
    wide = J.encode(noise, 90, J.TJPF_BGR, J.TJSAMP_420)
    assert len(wide) > 4 * 256 * 4 * 32
    batch = [jpegs[BIG], wide]
    wants = [want(j, R35) for j in batch]
    assert tj.filter2d_batch(batch, R35) == wants
    assert tj.filter2d(jpegs[BIG], R35) == wants[0]
    assert [bytes(v) for v in tj.invert_batch_result(tj.filter2d_batch_submit(batch, R35))] == wants
    twice = J.encode(R.filter2d(R.filter2d(J.decode(wide, J.TJPF_BGR), *R35), *R35), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert wants[1] != twice and wants[1] != J.encode(J.decode(wide, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_two_batches_in_flight_keep_their_own_kernels(tj, jpegs):
    w = np.array(R35[0], dtype=np.int16)
    t1 = tj.filter2d_batch_submit(jpegs, (w, R35[1]), border="replicate")
    w[:] = 0  # the kernel was copied at submit
    t2 = tj.filter2d_batch_submit(jpegs, G3)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, G3) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, R35, "replicate") for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_kernels_are_refused(tj, jpegs):
    with pytest.raises(ValueError):
        tj.filter2d(jpegs[0], np.full((3, 3), 1 / 9))
    with pytest.raises(ValueError):
        tj.filter2d_batch_submit(jpegs, np.ones((2, 2), int))
    with pytest.raises(ValueError):
        tj.filter2d(jpegs[0], G3, border="wrap")
    assert tj.filter2d(jpegs[0], G3) == want(jpegs[0], G3)


def test_conv_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.conv_worker import ConvWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = ConvWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, kernel=R35, **kw)
    try:
        assert bytes(w(j)) == want(j, R35)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, R35), want(jpegs[0], R35)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, R35), want(jpegs[3], R35)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, R35) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], R35)
    finally:
        w.close()
    rng = np.random.default_rng(61)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    w = ConvWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, kernel=R35, border="replicate", **kw)
    try:
        assert bytes(w(frame.tobytes())) == R.filter2d(frame, *R35, "replicate").tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == R.filter2d(small, *R35, "replicate").tobytes()
        assert bytes(res[1]) == R.filter2d(frame, *R35, "replicate").tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == R.filter2d(frame, *R35, "replicate").tobytes() and isinstance(bad[1], Exception)
    finally:
        w.close()
    frames = [rng.integers(0, 256, (12, 10, 3), dtype=np.uint8) for _ in range(3)]
    w = ConvWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, kernel=G3, shape=(12, 10, 3), **kw)
    try:
        assert bytes(w(frames[0].tobytes())) == R.filter2d(frames[0], *G3).tobytes()
        out1 = np.empty(360, np.uint8)
        res = w.process_batch([f.tobytes() for f in frames], [None] * 3, [None, out1, None])
        assert res[1] is out1
        assert [bytes(r) for r in res] == [R.filter2d(f, *G3).tobytes() for f in frames]
        h = w.submit_batch([f.tobytes() for f in frames], [None] * 3, [None] * 3)
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [R.filter2d(f, *G3).tobytes() for f in frames]
    finally:
        w.close()
    with pytest.raises(ValueError):
        ConvWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, kernel=np.full((3, 3), 1 / 9), **kw)


def test_invert_and_lut_are_unchanged_after_conv_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.filter2d(j, G3) == want(j, G3)
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert tj.filter2d(j, G3) == want(j, G3)
    t = tables.gamma(2.2)
    for x in jpegs:
        lut_want = J.encode(t[J.decode(x, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
        assert tj.lut(x, t) == lut_want
    assert tj.filter2d(j, G3) == want(j, G3)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a kernel
    img = J.decode(j, J.TJPF_BGR)
    assert tj.encode(img) == J.encode(img, 85, J.TJPF_BGR, J.TJSAMP_422)  # an encode too: it reads d_pix_ again
