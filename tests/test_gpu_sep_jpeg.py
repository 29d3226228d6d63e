"""The separable filter on the JPEG path (``TurboJPEG.sep_filter2d*``, ``blur*``, ``filter_batch*`` with a
``Separable``, chains with a sep step, ``SepWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_sep_ref.py`` on the BGR frame.  Whole JPEG byte strings
are compared, nothing less.  The inputs are ``tests/test_gpu_mix_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4
and grayscale, sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_sep as CS
import _conv_ref as C
import _rank_ref as R
import _sep_ref as S
from oracle import jpeg as J
from vfilter import Separable, tables
from vfilter import kernels as K
from vfilter.filters import Chain, Table
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (kx, ky, shift, divisor, rounding, border)
BOX5 = (np.ones(5, np.int64), np.ones(5, np.int64), 0, 25, "half_even", "reflect101")
G31 = (K.gaussian_taps(31, 5.0)[0].astype(np.int64), K.gaussian_taps(31, 5.0)[0].astype(np.int64), 16, 1, "half_up",
       "reflect101")
RAND = S.kernel_set()["rand15x5"][:2] + (7, 1, "half_even", "replicate")
ER35 = R.element_set()["rect3x5"]
FILTERS = {"box5": BOX5, "gauss31": G31, "rand15x5": RAND}

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
    key = (j, filt[0].tobytes(), filt[1].tobytes()) + tuple(filt[2:]) + (quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = S.sep(J.decode(j, J.TJPF_BGR, flags), *filt)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def sep_of(filt) -> Separable:
    kx, ky, shift, divisor, rounding, border = filt
    return Separable((kx, 0), (ky, 0), shift, divisor, rounding, border)


@pytest.mark.parametrize("fname", sorted(FILTERS))
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j, filt = jpegs[i], FILTERS[fname]
    assert tj.sep_filter2d(j, sep_of(filt), jpeg_subsample=out_ss) == want(j, filt, subsample=out_ss), (INPUTS[i], out_ss)


def test_mixed_batch_blur_and_the_one_step_chain(tj, jpegs):
    got = tj.blur_batch(jpegs, 5)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, BOX5), INPUTS[i]
    assert tj.chain_batch(jpegs, [Separable.box(5)]) == got  # tj.blur is the one-step tj.chain
    assert tj.filter_batch(jpegs, Separable.box(5)) == got
    assert tj.sep_filter2d_batch(jpegs, np.ones(5), np.ones(5), divisor=25) == got
    assert tj.blur_batch([], 5) == []
    j = jpegs[BIG]
    assert tj.blur(j, 5) == want(j, BOX5) == tj.chain(j, Chain(Separable.box(5)))
    assert tj.blur(j, (3, 9), border="replicate") == want(j, (np.ones(3, np.int64), np.ones(9, np.int64), 0, 27, "half_even",
                                                             "replicate"))
    assert tj.sep_filter2d(j, Separable.gaussian(31, 5.0)) == want(j, G31)
    ends = S.kernel_set()["ends9"]
    he, hu = ends[:2] + (1, 1, "half_even", "reflect101"), ends[:2] + (1, 1, "half_up", "reflect101")
    assert want(j, he) != want(j, hu)  # the rounding shows in the bytes
    assert tj.sep_filter2d(j, ends[0], ends[1], shift=1) == want(j, he)
    assert tj.sep_filter2d(j, ends[0], ends[1], shift=1, rounding="half_up") == want(j, hu)


def test_turbojpeg_2_another_quality_and_the_identity(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).blur(j, 5) == want(j, BOX5, tj_version=2)
    assert tj.blur(j, 5, quality=60) == want(j, BOX5, quality=60)
    assert tj.sep_filter2d(j, sep_of(G31), quality=97, jpeg_subsample=J.TJSAMP_420) == want(j, G31, 97, J.TJSAMP_420)
    plain = J.encode(J.decode(j, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)
    ident = np.zeros(31, np.int64)
    ident[15] = 1
    assert tj.sep_filter2d(j, ident, ident) == plain  # the plain decode -> encode round trip
    assert tj.blur(j, 1) == plain


def test_a_chain_with_a_sep_step(tj, jpegs):
    """A blur into a threshold, and an unsharp mask from a 15 x 15 mean, between one decode and one encode."""
    from vfilter.filters import Combine
    bt = [("sep", 0) + BOX5, ("table", 1, CR.threshold_table(128))]
    un = [("sep", 0, np.ones(15, np.int64), np.ones(15, np.int64), 0, 225, "half_even", "reflect101"), ("bin", "subtract", 0, 1),
          ("bin", "add", 0, 2)]
    chains = [(bt, Chain([Separable.box(5), Table(CR.threshold_table(128))])),
              (un, Chain(Combine("add", None, Combine("subtract", None, Separable.box(15)))))]
    for prog, c in chains:
        got = tj.chain_batch(jpegs, c)
        for i, (g, j) in enumerate(zip(got, jpegs)):
            ref = J.encode(CS.run(J.decode(j, J.TJPF_BGR), prog), 85, J.TJPF_BGR, J.TJSAMP_422)
            assert g == ref, (INPUTS[i], len(prog))


def test_a_resynchronised_batch_is_filtered_once(tj, jpegs, monkeypatch):
    """With one queued span pass the decode checks report the sync unconverged at the wait; the
    remaining passes, every decode stage after them, the filter and the encode run again.  The
    result is the filter applied once: not twice, not zero times."""
    monkeypatch.setenv("VF_JPEG_SYNC", "pass")
    monkeypatch.setenv("VF_JPEG_SYNC_G", "4")
    monkeypatch.setenv("VF_JPEG_SYNC_QUEUED", "1")
    noise = np.random.default_rng(81).integers(0, 256, (512, 640, 3), dtype=np.uint8)
    wide = J.encode(noise, 90, J.TJPF_BGR, J.TJSAMP_420)
    assert len(wide) > 4 * 256 * 4 * 32
    batch = [jpegs[BIG], wide]
    wants = [want(j, BOX5) for j in batch]
    assert tj.blur_batch(batch, 5) == wants
    assert tj.blur(jpegs[BIG], 5) == wants[0]
    assert [bytes(v) for v in tj.invert_batch_result(tj.filter_batch_submit(batch, Separable.box(5)))] == wants
    once = S.sep(J.decode(wide, J.TJPF_BGR), *BOX5)
    twice = J.encode(S.sep(once, *BOX5), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert wants[1] != twice and wants[1] != J.encode(J.decode(wide, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_three_batches_in_flight_keep_their_own_taps(tj, jpegs):
    kx, ky = np.array(RAND[0]), np.array(RAND[1])
    sep = Separable(kx, ky, shift=7, border="replicate")
    t1 = tj.filter_batch_submit(jpegs, sep)
    kx[:] = 0  # the taps were copied when the Separable was built ...
    ky[:] = 0
    rx, ry = np.ascontiguousarray(G31[0], np.int16), np.ascontiguousarray(G31[1], np.int16)
    t_raw = tj.ctx.jpeg_sep_submit(jpegs, rx, ry, 16, 1, 1, 0, 85, J.TJSAMP_422, 0)
    rx[:] = 0  # ... and again by the library at submit: these arrays went straight to the C call
    ry[:] = 0
    t2 = tj.filter_batch_submit(jpegs, Separable.box(5))
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, BOX5) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, RAND) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, G31) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_filters_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.blur(jpegs[0], 4)
    with pytest.raises(ValueError):
        tj.sep_filter2d(jpegs[0], np.full(3, 1 / 3))
    with pytest.raises(ValueError):
        tj.sep_filter2d_batch(jpegs, [1, 2, 1], rounding="nearest")
    ones = np.ones(33, np.int16)
    with pytest.raises(vfilter.VFilterError, match="odd and at most 31"):
        tj.ctx.jpeg_sep(jpegs, ones, ones[:3], 0, 1, 0, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="divisor=6"):
        tj.ctx.jpeg_sep_submit(jpegs, ones[:3], ones[:3], 0, 6, 0, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="together"):
        tj.ctx.jpeg_sep(jpegs, ones[:3], ones[:3], 2, 9, 0, 0, 85, J.TJSAMP_422, 0)
    assert tj.blur(jpegs[0], 5) == want(jpegs[0], BOX5)


def test_jpeg_bench_sep_runs(tj, jpegs):
    ms, stages = tj.ctx.jpeg_bench_sep([jpegs[BIG]] * 2, np.ones(5, np.int16), np.ones(5, np.int16), 0, 25, 0, 0, 85,
                                       J.TJSAMP_422, 0, iters=2)
    assert ms > 0 and isinstance(stages, dict)


def test_sep_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.sep_worker import SepWorker, sep_from_options
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = SepWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, sep=sep_from_options(box=[5]), **kw)
    try:
        assert bytes(w(j)) == want(j, BOX5)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, BOX5), want(jpegs[0], BOX5)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, BOX5), want(jpegs[3], BOX5)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, BOX5) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], BOX5)
    finally:
        w.close()
    rng = np.random.default_rng(63)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    w = SepWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, sep=sep_from_options(gaussian=(31, 5.0)), **kw)
    try:
        assert bytes(w(frame.tobytes())) == S.sep(frame, *G31).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        gray = rng.integers(0, 256, (12, 10), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == S.sep(small, *G31).tobytes() and bytes(res[1]) == S.sep(frame, *G31).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == S.sep(frame, *G31).tobytes() and isinstance(bad[1], Exception)
        res = w.process_batch([gray.tobytes()], [wire.FrameMeta(0, 120, [12, 10])], [None])  # a 1-channel frame works
        assert bytes(res[0]) == S.sep(gray, *G31).tobytes()
    finally:
        w.close()
    with pytest.raises(ValueError):
        SepWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, sep="box", **kw)
    for bad in (dict(), dict(box=[5], gaussian=(5, 1.0)), dict(box=[4]), dict(box=[5], shift=2), dict(box=[5], divisor=3),
                dict(gaussian=(5, 1.0), divisor=3), dict(gaussian=(5.5, 1.0)), dict(ky_npy="x.npy"),
                dict(box=[5], border="wrap"), dict(box=[5], rounding="nearest"), dict(box=[3, 5, 7])):
        with pytest.raises(ValueError):
            sep_from_options(**bad)
    assert sep_from_options(box=[5, 3], divisor=1).divisor == 1 and sep_from_options(box=[5, 3]).divisor == 15


def test_the_other_filters_are_unchanged_after_sep_calls(tj, jpegs):
    j = jpegs[BIG]
    g3 = C.kernel_set()["gaussian3"]
    assert tj.blur(j, 5) == want(j, BOX5)
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert tj.sep_filter2d(j, sep_of(G31)) == want(j, G31)
    t = tables.gamma(2.2)
    for x in jpegs:
        assert tj.lut(x, t) == J.encode(t[J.decode(x, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.blur(j, 5) == want(j, BOX5)
    assert tj.filter2d(j, g3) == J.encode(C.filter2d(J.decode(j, J.TJPF_BGR), *g3), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.erode(j, ER35) == J.encode(R.erode(J.decode(j, J.TJPF_BGR), ER35), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.blur(j, 5) == want(j, BOX5)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a separable filter
    img = J.decode(j, J.TJPF_BGR)
    assert tj.encode(img) == J.encode(img, 85, J.TJPF_BGR, J.TJSAMP_422)  # an encode too: it reads d_pix_ again
