"""Filter chains on the JPEG path (``TurboJPEG.chain*``, ``morphology_ex*``, ``ChainWorker``)
against the oracle composition

    oracle.jpeg.encode(run(oracle.jpeg.decode(j, TJPF_BGR, flags), prog), quality, TJPF_BGR, subsample, flags, tj_version)

with ``run`` the numpy interpreter of ``tests/_chain_ref.py`` on the BGR frame: one decode and one
encode around the whole program.  Whole JPEG byte strings are compared, nothing less.  The inputs
are ``tests/test_gpu_rank_jpeg.py``'s: 4:2:2, 4:2:0, 4:4:4 and grayscale, sizes that are not whole
MCUs and one of several kernel tiles.
"""
import numpy as np
import pytest

import _chain_ref as CR
import _conv_ref as C
import _rank_ref as R
from _chain_build import to_chain
from oracle import jpeg as J
from vfilter import tables
from vfilter.filters import Chain, Invert, Morph, Rank, Table
from vfilter.jpeg import TurboJPEG

pytestmark = pytest.mark.gpu

# (input subsampling, width, height)
INPUTS = [(J.TJSAMP_422, 16, 8), (J.TJSAMP_422, 17, 13), (J.TJSAMP_422, 250, 130), (J.TJSAMP_420, 17, 13),
          (J.TJSAMP_444, 9, 9), (J.TJSAMP_GRAY, 33, 17)]
BIG = 2  # the 250 x 130 4:2:2 input
G3 = C.kernel_set()["gaussian3"]
ER35 = R.element_set()["rect3x5"]


def progs(border="constant"):
    return CR.program_set(border, 3)


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    return [J.encode(J.synthetic_scene(90 + i, h, w), 90, J.TJPF_BGR, ss) for i, (ss, w, h) in enumerate(INPUTS)]


_want_cache = {}


def want(j, name, border="constant", quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    key = (j, name, border, quality, subsample, flags, tj_version)
    if key not in _want_cache:
        img = CR.run(J.decode(j, J.TJPF_BGR, flags), progs(border)[name])
        _want_cache[key] = J.encode(img, quality, J.TJPF_BGR, subsample, flags, tj_version)
    return _want_cache[key]


def chain_of(name, border="constant"):
    return to_chain(progs(border)[name])


@pytest.mark.parametrize("name", ["edges", "gradient_random7"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_to_each_output_form(tj, jpegs, i, out_ss, name):
    j = jpegs[i]
    assert tj.chain(j, chain_of(name), jpeg_subsample=out_ss) == want(j, name, subsample=out_ss), (INPUTS[i], out_ss)


@pytest.mark.parametrize("border", ["reflect101", "replicate", "constant"])
def test_mixed_batch(tj, jpegs, border):
    for name in ("gradient_random7", "blackhat3_it2", "dog", "eight", "diamond", "corner5_reversed"):
        got = tj.chain_batch(jpegs, chain_of(name, border))
        for i, (g, j) in enumerate(zip(got, jpegs)):
            assert g == want(j, name, border), (name, INPUTS[i], border)
    assert tj.chain_batch([], chain_of("edges")) == [] and tj.morphology_ex_batch([], "open") == []


def test_every_program_on_the_big_input(tj, jpegs):
    j = jpegs[BIG]
    for name in sorted(progs()):
        assert tj.chain(j, chain_of(name)) == want(j, name), name


@pytest.mark.parametrize("op", CR.MORPH_OPS)
def test_morphology_ex(tj, jpegs, op):
    j = jpegs[BIG]
    img = J.decode(j, J.TJPF_BGR)
    for border in CR.BORDERS:
        ref = J.encode(CR.run(img, CR.morph(op, ER35, 1, border)), 85, J.TJPF_BGR, J.TJSAMP_422)
        assert tj.morphology_ex(j, op, ER35, border=border) == ref, (op, border)
    ref2 = J.encode(CR.run(img, CR.morph(op, R.rect(3), 2)), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.morphology_ex_batch([j, j], op, None, 2) == [ref2, ref2]  # element=None: the 3 x 3 rectangle


def test_turbojpeg_2_and_another_quality(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).chain(j, chain_of("edges")) == want(j, "edges", tj_version=2)
    assert tj.chain(j, chain_of("edges"), quality=60) == want(j, "edges", quality=60)
    assert tj.chain(j, chain_of("dog"), quality=97, jpeg_subsample=J.TJSAMP_444) == want(j, "dog", quality=97,
                                                                                       subsample=J.TJSAMP_444)


def test_programs_that_are_one_filter_run_as_that_filter(tj, jpegs):
    # pointwise folds to one table: the fused colour stage, the same bytes as tj.lut with the composed table
    curves = CR.curves_table()
    composed = np.stack([CR.INVERT[curves[:, c][CR.INVERT]] for c in range(3)], axis=1)
    for j in jpegs:
        got = tj.chain(j, chain_of("pointwise"))
        assert got == tj.lut(j, composed) == want(j, "pointwise")
    assert tj.chain(jpegs[BIG], [Invert()]) == J.invert_jpeg(jpegs[BIG]) == tj.invert(jpegs[BIG])
    # one step: the single filter's bytes
    for j in jpegs:
        assert tj.chain(j, [Rank.erode(ER35)]) == tj.erode(j, ER35)
        assert tj.morphology_ex(j, "dilate", ER35, border="replicate") == tj.dilate(j, ER35, border="replicate")
        assert tj.chain(j, Chain([Rank.median(3)])) == tj.median_blur(j, 3)


def test_a_resynchronised_batch_is_filtered_once(tj, jpegs, monkeypatch):
    """With one queued span pass the decode checks report the sync unconverged at the wait; the
    remaining passes, every decode stage after them, the program and the encode run again.  The
    program reuses the decoded frame's buffer, so a second run on what the first left, or an
    encoder reading an intermediate value, shows: the result is the program applied once."""
    monkeypatch.setenv("VF_JPEG_SYNC", "pass")
    monkeypatch.setenv("VF_JPEG_SYNC_G", "4")
    monkeypatch.setenv("VF_JPEG_SYNC_QUEUED", "1")
    noise = np.random.default_rng(81).integers(0, 256, (512, 640, 3), dtype=np.uint8)
    wide = J.encode(noise, 90, J.TJPF_BGR, J.TJSAMP_420)
    assert len(wide) > 4 * 256 * 4 * 32
    batch = [jpegs[BIG], wide]
    for name in ("gradient_random7", "blackhat3_it2"):
        wants = [want(j, name) for j in batch]
        c = chain_of(name)
        assert tj.chain_batch(batch, c) == wants
        assert tj.chain(jpegs[BIG], c) == wants[0]
        assert [bytes(v) for v in tj.invert_batch_result(tj.chain_batch_submit(batch, c))] == wants
        once = CR.run(J.decode(wide, J.TJPF_BGR), progs()[name])
        twice = J.encode(CR.run(once, progs()[name]), 85, J.TJPF_BGR, J.TJSAMP_422)
        assert wants[1] != twice and wants[1] != J.encode(J.decode(wide, J.TJPF_BGR), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_three_batches_in_flight_keep_their_own_filters(tj, jpegs):
    thr = CR.threshold_table().copy()
    e = np.ones((3, 3), np.uint8)
    c = Chain([Rank.median(3), Morph("gradient", e), Table(thr)])  # "edges"
    t1 = tj.chain_batch_submit(jpegs, c)
    # the arrays of the program's steps, straight to the C call: overwritten right after the submit
    steps = [list(st) for st in c.steps]
    mine = {}
    for st in steps:
        if st[4] is not None:
            st[4] = mine.setdefault(id(st[4]), np.array(np.frombuffer(st[4], np.uint8) if isinstance(st[4], bytes) else st[4]))
    t_raw = tj.ctx.jpeg_chain_submit(jpegs, [tuple(st) for st in steps], 85, J.TJSAMP_422, 0)
    for a in mine.values():
        a[...] = 0
    thr[:] = 0
    e[:] = 0
    t2 = tj.filter_batch_submit(jpegs, Rank.dilate(R.element_set()["random7"], "replicate"))
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == \
        [J.encode(R.dilate(J.decode(j, J.TJPF_BGR), R.element_set()["random7"], "replicate"), 85, J.TJPF_BGR, J.TJSAMP_422)
         for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, "edges") for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t_raw)] == [want(j, "edges") for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_programs_are_refused(tj, jpegs):
    with pytest.raises(ValueError):
        tj.chain(jpegs[0], [])
    with pytest.raises(ValueError):
        tj.chain_batch(jpegs, [Invert()] * 9)
    with pytest.raises(ValueError):
        tj.morphology_ex(jpegs[0], "gradient", None, 4)
    with pytest.raises(ValueError):
        tj.morphology_ex_batch(jpegs, "open", np.ones((2, 2)))
    with pytest.raises(ValueError):
        tj.chain_batch_submit(jpegs, [Rank.erode(None, "wrap")])
    assert tj.chain(jpegs[0], chain_of("edges")) == want(jpegs[0], "edges")


def test_chain_worker_jpeg_and_raw(jpegs):
    from vfilter import wire
    from vfilter.chain_worker import ChainWorker, morph_from_options
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = ChainWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, chain=chain_of("edges"), **kw)
    try:
        assert bytes(w(j)) == want(j, "edges")
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, "edges"), want(jpegs[0], "edges")]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, "edges"), want(jpegs[3], "edges")]
        corrupt = j[:len(j) // 2]  # it fails alone
        res = w.process_batch([j, corrupt, jpegs[1]], [None] * 3, [None] * 3)
        assert bytes(res[0]) == want(j, "edges") and isinstance(res[1], Exception) and bytes(res[2]) == want(jpegs[1], "edges")
    finally:
        w.close()
    rng = np.random.default_rng(62)
    frame = rng.integers(0, 256, (480, 480, 3), dtype=np.uint8)  # the reference's raw frame (inverter.py:34)
    bh = CR.morph("blackhat", R.cross(5), 1, "replicate")
    w = ChainWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, chain=morph_from_options("blackhat", "cross", (5,), 1, "replicate"),
                    **kw)
    try:
        assert bytes(w(frame.tobytes())) == CR.run(frame, bh).tobytes()
        small = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
        metas = [wire.FrameMeta(0, small.nbytes, [12, 10, 3]), wire.FrameMeta(1, frame.nbytes, None)]
        res = w.process_batch([small.tobytes(), frame.tobytes()], metas, [None, None])  # the shape from the metadata
        assert bytes(res[0]) == CR.run(small, bh).tobytes()
        assert bytes(res[1]) == CR.run(frame, bh).tobytes()
        bad = w.process_batch([frame.tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B is not 480 x 480 x 3
        assert bytes(bad[0]) == CR.run(frame, bh).tobytes() and isinstance(bad[1], Exception)
    finally:
        w.close()
    frames = [rng.integers(0, 256, (12, 10, 3), dtype=np.uint8) for _ in range(3)]
    dog = progs("reflect101")["dog"]
    w = ChainWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, chain=to_chain(dog), shape=(12, 10, 3), **kw)
    try:
        assert bytes(w(frames[0].tobytes())) == CR.run(frames[0], dog).tobytes()
        out1 = np.empty(360, np.uint8)
        res = w.process_batch([f.tobytes() for f in frames], [None] * 3, [None, out1, None])
        assert res[1] is out1
        assert [bytes(r) for r in res] == [CR.run(f, dog).tobytes() for f in frames]
        h = w.submit_batch([f.tobytes() for f in frames], [None] * 3, [None] * 3)
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [CR.run(f, dog).tobytes() for f in frames]
    finally:
        w.close()
    with pytest.raises(ValueError):
        ChainWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, chain="open", **kw)


def test_the_other_filters_are_unchanged_after_chain_calls(tj, jpegs):
    j = jpegs[BIG]
    c = chain_of("eight")  # the program with the most buffers
    assert tj.chain(j, c) == want(j, "eight")
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert tj.chain(j, c) == want(j, "eight")
    t = tables.gamma(2.2)
    for x in jpegs:
        assert tj.lut(x, t) == J.encode(t[J.decode(x, J.TJPF_BGR)], 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.chain(j, c) == want(j, "eight")
    assert tj.filter2d(j, G3) == J.encode(C.filter2d(J.decode(j, J.TJPF_BGR), *G3), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.chain(j, c) == want(j, "eight")
    assert tj.erode(j, ER35) == J.encode(R.erode(J.decode(j, J.TJPF_BGR), ER35), 85, J.TJPF_BGR, J.TJSAMP_422)
    assert tj.chain(j, c) == want(j, "eight")
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last ran a chain
    img = J.decode(j, J.TJPF_BGR)
    assert tj.chain(j, c) == want(j, "eight")
    assert tj.encode(img) == J.encode(img, 85, J.TJPF_BGR, J.TJSAMP_422)  # an encode too: it reads d_pix_ again
