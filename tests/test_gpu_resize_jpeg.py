"""The resize on the JPEG path (``TurboJPEG.resize``, ``resize_batch``, ``filter_batch*`` with a ``Resize``, chains with
a resize step, ``ResizeWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_resize_ref.py`` on the BGR frame.  Whole JPEG byte strings are compared,
nothing less: the header carries the RESULT's size, and the block counts and the MCU padding follow it.  48 x 32 ->
23 x 17 and 24 x 16 -> 50 x 35 leave whole MCUs for sizes that are padded under 4:2:0, 4:2:2 and 4:4:4 alike.
"""
import numpy as np
import pytest

import _resize_ref as R
from oracle import jpeg as J
from vfilter import Resize
from vfilter.filters import Chain, Invert
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (input subsampling, width, height)
INPUTS = [(J.TJSAMP_422, 48, 32), (J.TJSAMP_420, 24, 16), (J.TJSAMP_444, 17, 13), (J.TJSAMP_GRAY, 33, 17), (J.TJSAMP_422, 130, 70)]
SHRINK, GROW = Resize((23, 17)), Resize((50, 35))
SCALED = Resize(fx=0.5, fy=0.75)  # each frame from its own size; 48 x 32 and 130 x 70 are not 2 x 2, so linear stays linear


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    return [J.encode(J.synthetic_scene(70 + i, h, w), 90, J.TJPF_BGR, ss) for i, (ss, w, h) in enumerate(INPUTS)]


_want_cache = {}


def ref(img, f: Resize):
    return R.resize(img, f.dsize, f.fx, f.fy, f.interp_code)


def want(j, f: Resize, quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    key = (j, f.args, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        _want_cache[key] = J.encode(ref(J.decode(j, J.TJPF_BGR, flags), f), quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


@pytest.mark.parametrize("out_ss", [J.TJSAMP_420, J.TJSAMP_422, J.TJSAMP_444])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_results_with_mcu_padding_under_every_sampling(tj, jpegs, interp, out_ss):
    for j, dsize in [(jpegs[0], (23, 17)), (jpegs[1], (50, 35))]:
        f = Resize(dsize, interpolation=interp)
        got = tj.filter_batch([j], f, jpeg_subsample=out_ss)[0]
        assert got == want(j, f, subsample=out_ss), (dsize, interp, out_ss)
        assert tj.decode_header(got)[:2] == dsize  # the header carries the new size
        assert J.decode(got).shape[:2] == (dsize[1], dsize[0])


def test_a_batch_of_mixed_input_sizes_with_one_fx_fy(tj, jpegs):
    got = tj.resize_batch(jpegs, fx=0.5, fy=0.75)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        _, w, h = INPUTS[i]
        assert g == want(j, SCALED), INPUTS[i]
        assert tj.decode_header(g)[:2] == SCALED.out_size(w, h)
    assert tj.filter_batch(jpegs, SCALED) == got and tj.chain_batch(jpegs, [SCALED]) == got  # a resize is the one-step chain
    assert tj.resize_batch([], (4, 4)) == []
    area = Resize(fx=0.5, fy=0.5, interpolation="area")
    assert tj.resize_batch(jpegs, fx=0.5, fy=0.5, interpolation="area") == [want(j, area) for j in jpegs]
    j = jpegs[4]
    assert tj.resize(j, (23, 17)) == want(j, SHRINK) != want(j, Resize((23, 17), interpolation="nearest"))
    assert tj.resize(j, (50, 35), quality=60, jpeg_subsample=J.TJSAMP_420) == want(j, GROW, 60, J.TJSAMP_420)
    assert tj.resize(j, None, 2, 2, "nearest") == want(j, Resize(fx=2, fy=2, interpolation="nearest"))


def test_the_submit_and_wait_forms(tj, jpegs):
    t1 = tj.filter_batch_submit(jpegs, GROW)
    t2 = tj.filter_batch_submit(jpegs, SCALED)
    t_raw = tj.ctx.jpeg_resize_submit(jpegs, *SHRINK.args, 85, J.TJSAMP_422, 0)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, SCALED) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, GROW) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, SHRINK) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]
    assert tj.ctx.jpeg_resize(jpegs, 23, 17, 0.0, 0.0, 1, 85, J.TJSAMP_422, 0) == [want(j, SHRINK) for j in jpegs]
    # the same codec, a batch of the same inputs and another result size: the encoder's cached layout follows the size
    assert tj.filter_batch(jpegs, SHRINK) == [want(j, SHRINK) for j in jpegs]
    assert tj.filter_batch(jpegs, GROW) == [want(j, GROW) for j in jpegs]
    assert tj.invert_batch(jpegs) == [J.invert_jpeg(j) for j in jpegs]


def test_chains_with_a_resize_step(tj, jpegs):
    """Resize first, last and between; the value after the decoded frame may be larger than the frame."""
    got = tj.chain_batch(jpegs, Chain([GROW, Invert()]))
    got2 = tj.chain_batch(jpegs, Chain([Invert(), SCALED]))
    got3 = tj.chain_batch(jpegs, Chain([Resize(fx=2, fy=2, interpolation="nearest"), Invert(), SHRINK]))
    for i, (g, g2, g3, j) in enumerate(zip(got, got2, got3, jpegs)):
        img = J.decode(j, J.TJPF_BGR)
        assert g == J.encode(255 - ref(img, GROW), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]
        assert g2 == J.encode(ref(255 - img, SCALED), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]
        up = 255 - R.resize(img, None, 2, 2, R.NEAREST)
        assert g3 == J.encode(ref(up, SHRINK), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]


def test_bad_filters_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.resize(jpegs[0], (0, 5))
    with pytest.raises(ValueError):
        tj.resize(jpegs[0], (5, 5), interpolation=2)
    with pytest.raises(vfilter.VFilterError, match="is not built"):
        tj.ctx.jpeg_resize(jpegs, 5, 5, 0.0, 0.0, 2, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="a side is 1 to 32767"):
        tj.ctx.jpeg_resize_submit(jpegs, 32768, 5, 0.0, 0.0, 1, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="frame 0: step 1: area from 48 x 32 to 23 x 17"):  # found when the frames are known
        tj.ctx.jpeg_resize(jpegs, 23, 17, 0.0, 0.0, 3, 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="a side of 0"):
        tj.ctx.jpeg_resize(jpegs, 0, 0, 0.01, 0.01, 1, 85, J.TJSAMP_422, 0)
    assert tj.resize(jpegs[0], (23, 17)) == want(jpegs[0], SHRINK)


def test_jpeg_bench_resize_runs(tj, jpegs):
    ms, stages = tj.ctx.jpeg_bench_resize([jpegs[4]] * 2, *GROW.args, 85, J.TJSAMP_422, 0, iters=2)
    assert ms > 0 and isinstance(stages, dict)


def test_resize_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.resize_worker import ResizeWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[4]
    w = ResizeWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, resize=SCALED, **kw)
    try:
        assert bytes(w(j)) == want(j, SCALED)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, SCALED), want(jpegs[0], SCALED)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, SCALED), want(jpegs[3], SCALED)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, SCALED) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], SCALED)
    finally:
        w.close()
    rng = np.random.default_rng(64)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    f = Resize(fx=0.3, fy=0.5)
    w = ResizeWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, resize=f, **kw)
    try:
        out = w(frame.tobytes())
        assert len(bytes(out)) == 144 * 240 * 3 and bytes(out) == ref(frame, f).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        gray = rng.integers(0, 256, (12, 10), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # a wire batch: the shape from the metadata
        assert bytes(res[0]) == ref(small, f).tobytes() and bytes(res[1]) == ref(frame, f).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == ref(frame, f).tobytes() and isinstance(bad[1], Exception)
        res = w.process_batch([gray.tobytes()], [wire.FrameMeta(0, 120, [12, 10])], [None])  # a 1-channel frame works
        assert bytes(res[0]) == ref(gray, f).tobytes()
    finally:
        w.close()
    with pytest.raises(ValueError):
        ResizeWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, resize="half", **kw)
