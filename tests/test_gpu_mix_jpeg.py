"""The colour matrix on the JPEG path (``TurboJPEG.transform*``, ``filter_batch*`` with a ``Mix``,
chains with a mix step, ``MixWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_mix_ref.py`` on the BGR frame.  Whole JPEG byte strings
are compared, nothing less.  The inputs are ``tests/test_gpu_rank_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4
and grayscale, sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _chain_ref_mix as CM
import _conv_ref as C
import _mix_ref as M
import _rank_ref as R
from oracle import jpeg as J
from vfilter import Mix, colors, tables
from vfilter.filters import Chain, Kernel, Rank
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (matrix, shift, rounding)
SEPIA = (M.mat([[34, 137, 70], [43, 176, 89], [48, 197, 101]]), 8, "half_even")
GRAY = (M.mat([[3735, 19235, 9798]] * 3), 15, "half_up")
SWAP = (M.mat(np.eye(3)[::-1], (0, -30, 30)), 0, "half_even")  # shift 0, with offsets
G3 = C.kernel_set()["gaussian3"]
ER35 = R.element_set()["rect3x5"]

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
    m, shift, rounding = filt
    key = (j, m.tobytes(), shift, rounding, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = M.mix(J.decode(j, J.TJPF_BGR, flags), m, shift, rounding)
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def mix_of(filt) -> Mix:
    return Mix((filt[0], filt[1]), filt[2])


def run(tj, j, filt, **kw):
    return tj.transform(j, (filt[0], filt[1]), rounding=filt[2], **kw)


@pytest.mark.parametrize("fname", ["sepia", "gray", "swap"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j = jpegs[i]
    filt = {"sepia": SEPIA, "gray": GRAY, "swap": SWAP}[fname]
    assert run(tj, j, filt, jpeg_subsample=out_ss) == want(j, filt, subsample=out_ss), (INPUTS[i], out_ss)


def test_mixed_batch_and_the_one_step_chain(tj, jpegs):
    for filt in (SEPIA, GRAY):
        got = tj.transform_batch(jpegs, (filt[0], filt[1]), rounding=filt[2])
        for i, (g, j) in enumerate(zip(got, jpegs)):
            assert g == want(j, filt), INPUTS[i]
        assert tj.chain_batch(jpegs, [mix_of(filt)]) == got  # tj.transform is the one-step tj.chain
        assert tj.filter_batch(jpegs, mix_of(filt)) == got
    assert tj.transform_batch([], colors.sepia()) == []
    j = jpegs[BIG]
    assert tj.transform(j, colors.sepia()) == want(j, SEPIA) == tj.chain(j, Chain(Mix(colors.sepia())))
    assert tj.transform(j, colors.gray()) == want(j, GRAY)  # the preset carries half_up
    he, hu = M.TIES + ("half_even",), M.TIES + ("half_up",)  # a matrix with many exact ties
    assert want(j, he) != want(j, hu)  # the rounding shows in the bytes
    assert tj.transform(j, M.TIES) == want(j, he) and tj.transform(j, M.TIES, rounding="half_up") == want(j, hu)


def test_turbojpeg_2_another_quality_and_the_identity(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).transform(j, colors.sepia()) == want(j, SEPIA, tj_version=2)
    assert tj.transform(j, colors.sepia(), quality=60) == want(j, SEPIA, quality=60)
    plain = J.encode(J.decode(j, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.transform(j, colors.identity()) == plain  # the plain decode -> encode round trip
    assert tj.transform(j, colors.swap_rb()) == J.encode(J.decode(j, J.TJPF_BGR)[..., ::-1], 85, J.TJPF_BGR, J.TJSAMP_422)


def test_a_chain_with_a_mix_step(tj, jpegs):
    """gray -> median3 -> gradient -> threshold, and a blur into sepia, between one decode and one encode."""
    import _chain_ref as CR
    el = R.element_set()
    edges = [("mix", 0) + GRAY, ("rank", 1, "median", 3, "replicate"), ("rank", 2, "dilate", el["rect3"], "constant"),
             ("rank", 2, "erode", el["rect3"], "constant"), ("bin", "subtract", 3, 4), ("table", 5, CR.threshold_table())]
    blur = [("conv", 0, G3[0], G3[1], "reflect101"), ("mix", 1) + SEPIA, ("bin", "max", 2, 1)]
    from vfilter.filters import Morph, Table
    chains = [(edges, Chain([mix_of(GRAY), Rank.median(3), Morph("gradient"), Table(CR.threshold_table())])),
              (blur, Chain.program([(Kernel(G3), 0), (mix_of(SEPIA), 1), ("max", 2, 1)]))]
    for prog, c in chains:
        got = tj.chain_batch(jpegs, c)
        for i, (g, j) in enumerate(zip(got, jpegs)):
            ref = J.encode(CM.run(J.decode(j, J.TJPF_BGR), prog), 85, J.TJPF_BGR, J.TJSAMP_422)
            assert g == ref, (INPUTS[i], len(prog))


def test_a_resynchronised_batch_is_filtered_once(tj, jpegs, monkeypatch):
    """With one queued span pass the decode checks report the sync unconverged at the wait; the
    remaining passes, every decode stage after them, the matrix and the encode run again.  The
    result is the matrix applied once: not twice, not zero times."""
    monkeypatch.setenv("VF_JPEG_SYNC", "pass")
    monkeypatch.setenv("VF_JPEG_SYNC_G", "4")
    monkeypatch.setenv("VF_JPEG_SYNC_QUEUED", "1")
    noise = np.random.default_rng(81).integers(0, 256, (512, 640, 3), dtype=np.uint8)
    wide = J.encode(noise, 90, J.TJPF_BGR, J.TJSAMP_420)
    assert len(wide) > 4 * 256 * 4 * 32
    batch = [jpegs[BIG], wide]
    wants = [want(j, SEPIA) for j in batch]
    assert tj.transform_batch(batch, colors.sepia()) == wants
    assert tj.transform(jpegs[BIG], colors.sepia()) == wants[0]
    assert [bytes(v) for v in tj.invert_batch_result(tj.filter_batch_submit(batch, mix_of(SEPIA)))] == wants
    once = M.mix(J.decode(wide, J.TJPF_BGR), *SEPIA)
    twice = J.encode(M.mix(once, *SEPIA), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert wants[1] != twice and wants[1] != J.encode(J.decode(wide, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_three_batches_in_flight_keep_their_own_matrices(tj, jpegs):
    m = np.array(SEPIA[0])
    mix = Mix((m, 8))
    t1 = tj.filter_batch_submit(jpegs, mix)
    m[:] = 0  # the matrix was copied when the Mix was built ...
    raw = np.ascontiguousarray(GRAY[0], np.int32)
    t_raw = tj.ctx.jpeg_mix_submit(jpegs, raw, 15, 1, 85, J.TJSAMP_422, 0)
    raw[:] = 0  # ... and again by the library at submit: this array went straight to the C call
    t2 = tj.filter_batch_submit(jpegs, mix_of(SWAP))
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, SWAP) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, SEPIA) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, GRAY) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_matrices_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.transform(jpegs[0], np.full((3, 3), 1 / 3))
    with pytest.raises(ValueError):
        tj.transform(jpegs[0], np.eye(4))
    with pytest.raises(ValueError):
        tj.transform_batch(jpegs, colors.sepia(), rounding="nearest")
    bad = np.ascontiguousarray(SEPIA[0], np.int32)
    bad[0, 0] = 40000
    with pytest.raises(vfilter.VFilterError, match="does not fit int16"):
        tj.ctx.jpeg_mix(jpegs, bad, 8, 0, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="unknown rounding 3"):
        tj.ctx.jpeg_mix_submit(jpegs, np.ascontiguousarray(SEPIA[0], np.int32), 8, 3, 85, J.TJSAMP_422, 0)
    assert tj.transform(jpegs[0], colors.sepia()) == want(jpegs[0], SEPIA)


def test_mix_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.mix_worker import MixWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = MixWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, mix=colors.gray(), **kw)
    try:
        assert bytes(w(j)) == want(j, GRAY)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, GRAY), want(jpegs[0], GRAY)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, GRAY), want(jpegs[3], GRAY)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, GRAY) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], GRAY)
    finally:
        w.close()
    rng = np.random.default_rng(62)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    w = MixWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, mix=Mix(colors.sepia()), **kw)
    try:
        assert bytes(w(frame.tobytes())) == M.mix(frame, *SEPIA).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == M.mix(small, *SEPIA).tobytes() and bytes(res[1]) == M.mix(frame, *SEPIA).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == M.mix(frame, *SEPIA).tobytes() and isinstance(bad[1], Exception)
        res = w.process_batch([bytes(120)], [wire.FrameMeta(0, 120, [12, 10])], [None])  # a 1-channel frame fails
        assert isinstance(res[0], Exception)
    finally:
        w.close()
    with pytest.raises(ValueError):
        MixWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, mix="gray", **kw)
    with pytest.raises(ValueError, match="H W 3"):
        MixWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, mix=colors.gray(), shape=(480, 480), **kw)


def test_the_other_filters_are_unchanged_after_mix_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.transform(j, colors.sepia()) == want(j, SEPIA)
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert tj.transform(j, colors.gray()) == want(j, GRAY)
    t = tables.gamma(2.2)
    for x in jpegs:
        assert tj.lut(x, t) == J.encode(t[J.decode(x, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.transform(j, colors.sepia()) == want(j, SEPIA)
    assert tj.erode(j, ER35) == J.encode(R.erode(J.decode(j, J.TJPF_BGR), ER35), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.transform(j, colors.sepia()) == want(j, SEPIA)
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a matrix
    img = J.decode(j, J.TJPF_BGR)
    assert tj.encode(img) == J.encode(img, 85, J.TJPF_BGR, J.TJSAMP_422)  # an encode too: it reads d_pix_ again
