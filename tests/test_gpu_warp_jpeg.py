"""The affine warp on the JPEG path (``TurboJPEG.flip``, ``TurboJPEG.warp_affine``, ``filter_batch*`` with a ``Warp``,
chains with a warp step, ``WarpWorker``) against the oracle composition

    oracle.jpeg.encode(ref(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``ref`` the numpy reference of ``tests/_warp_ref.py`` on the BGR frame.  Whole JPEG byte strings are compared,
nothing less.  The inputs are ``tests/test_gpu_clahe_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4 and grayscale (decoded to
three equal channels), sizes that are not whole MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _warp_ref as R
from oracle import jpeg as J
from vfilter import Warp, tables, warps
from vfilter.filters import Chain, Invert
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

TILT = warps.rotation((20, 11), 5.0, 1.1)
FILTERS = {
    "flip_h": Warp(flip="h", interpolation="nearest"),
    "flip_both": Warp(flip="both", interpolation="nearest"),
    "tilt_linear_reflect": Warp(TILT, border="reflect101"),
    "shift_constant_colour": Warp(warps.translation(2.5, -1.25), border="constant", border_value=(200, 100, 50)),
}

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


def ref(img, f: Warp):
    return R.warp(img, f.m, f.mode, f.interp_code, f.border_code, f.value)


def want(j, f: Warp, quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    key = (j, f.args, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        _want_cache[key] = J.encode(ref(J.decode(j, J.TJPF_BGR, flags), f), quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


@pytest.mark.parametrize("fname", sorted(FILTERS))
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, fname):
    j, f = jpegs[i], FILTERS[fname]
    assert tj.filter_batch([j], f, jpeg_subsample=out_ss)[0] == want(j, f, subsample=out_ss), (INPUTS[i], out_ss)


def test_mixed_batch_and_the_drop_ins(tj, jpegs):
    """One flip value mirrors a batch of mixed sizes: the map is resolved for every frame."""
    f = FILTERS["flip_h"]
    got = tj.filter_batch(jpegs, f)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, f), INPUTS[i]
    assert tj.chain_batch(jpegs, [f]) == got  # a warp is the one-step chain
    assert tj.filter_batch([], f) == []
    j = jpegs[BIG]
    assert tj.flip(j, 1) == want(j, f) == tj.flip(j, "h")
    assert tj.flip(j, -1) == want(j, FILTERS["flip_both"])
    assert tj.flip(j, 0) == want(j, Warp(flip="v", interpolation="nearest"))
    assert J.decode(tj.flip(j, 1, quality=100, jpeg_subsample=J.TJSAMP_444)).shape == J.decode(j).shape
    assert tj.warp_affine(j, TILT, border="reflect101") == want(j, FILTERS["tilt_linear_reflect"])
    assert tj.warp_affine(j, warps.translation(2.5, -1.25), border_value=(200, 100, 50)) == want(j, FILTERS["shift_constant_colour"])
    near = Warp(TILT, interpolation="nearest")
    assert tj.warp_affine(j, TILT, flags="nearest") == want(j, near) != want(j, Warp(TILT))
    assert tj.warp_affine(j, TILT, quality=60, jpeg_subsample=J.TJSAMP_420) == want(j, Warp(TILT), 60, J.TJSAMP_420)
    assert len({want(j, f) for f in FILTERS.values()}) == len(FILTERS)  # the filters differ in the bytes


def test_the_submit_and_wait_forms(tj, jpegs):
    f1, f2 = FILTERS["tilt_linear_reflect"], FILTERS["flip_both"]
    t1 = tj.filter_batch_submit(jpegs, f1)
    t2 = tj.filter_batch_submit(jpegs, f2)
    t_raw = tj.ctx.jpeg_warp_submit(jpegs, *FILTERS["shift_constant_colour"].args, 85, J.TJSAMP_422, 0)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, f2) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, f1) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, FILTERS["shift_constant_colour"]) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]
    assert tj.ctx.jpeg_warp(jpegs, None, 1, 1, 2, (0, 0, 0), 85, J.TJSAMP_422, 0) == [want(j, FILTERS["flip_h"]) for j in jpegs]


def test_a_chain_with_a_warp_step(tj, jpegs):
    """A flip into an inversion, and an inversion into a tilt, between one decode and one encode."""
    f = FILTERS["tilt_linear_reflect"]
    got = tj.chain_batch(jpegs, Chain([FILTERS["flip_h"], Invert()]))
    got2 = tj.chain_batch(jpegs, Chain([Invert(), f]))
    for i, (g, g2, j) in enumerate(zip(got, got2, jpegs)):
        img = J.decode(j, J.TJPF_BGR)
        assert g == J.encode(255 - img[:, ::-1], 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]
        assert g2 == J.encode(ref(255 - img, f), 85, J.TJPF_BGR, J.TJSAMP_422), INPUTS[i]


def test_bad_filters_are_refused(tj, jpegs):
    import vfilter
    with pytest.raises(ValueError):
        tj.flip(jpegs[0], "diagonal")
    with pytest.raises(ValueError):
        tj.warp_affine(jpegs[0], np.eye(3))
    with pytest.raises(vfilter.VFilterError, match="mode=4"):
        tj.ctx.jpeg_warp(jpegs, None, 4, 0, 2, (0, 0, 0), 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match="unknown border 3"):
        tj.ctx.jpeg_warp_submit(jpegs, None, 1, 0, 3, (0, 0, 0), 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match=r"value\[2\]=256"):
        tj.ctx.jpeg_warp(jpegs, None, 1, 0, 2, (0, 0, 256), 85, J.TJSAMP_422, 0)
    with pytest.raises(vfilter.VFilterError, match=r"m\[2\]"):  # a frame's limit: found when the frames are known
        tj.ctx.jpeg_warp(jpegs, (1, 0, 3e6, 0, 1, 0), 0, 0, 2, (0, 0, 0), 85, J.TJSAMP_422, 0)
    assert tj.flip(jpegs[0], 1) == want(jpegs[0], FILTERS["flip_h"])


def test_jpeg_bench_warp_runs(tj, jpegs):
    ms, stages = tj.ctx.jpeg_bench_warp([jpegs[BIG]] * 2, *FILTERS["tilt_linear_reflect"].args, 85, J.TJSAMP_422, 0, iters=2)
    assert ms > 0 and isinstance(stages, dict)


def test_warp_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.warp_worker import WarpWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    f = FILTERS["flip_h"]
    w = WarpWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, warp=f, **kw)
    try:
        assert bytes(w(j)) == want(j, f)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, f), want(jpegs[0], f)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, f), want(jpegs[3], f)]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, f) and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], f)
    finally:
        w.close()
    rng = np.random.default_rng(63)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    f = Warp(warps.rotation((239.5, 239.5), 5.0, 1.1), border="replicate")
    w = WarpWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, warp=f, **kw)
    try:
        assert bytes(w(frame.tobytes())) == ref(frame, f).tobytes()
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
        WarpWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, warp="h", **kw)


def test_the_other_filters_are_unchanged_after_warp_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.flip(j, 1) == want(j, FILTERS["flip_h"])
    assert tj.invert_batch(jpegs) == [J.invert_jpeg(x) for x in jpegs]
    t = tables.gamma(2.2)
    assert tj.lut(j, t) == J.encode(t[J.decode(j, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.flip(j, 1) == want(j, FILTERS["flip_h"])
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a warp
