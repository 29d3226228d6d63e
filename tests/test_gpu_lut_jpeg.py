"""The table filter on the JPEG path (``TurboJPEG.lut*``, ``LutWorker``) against the oracle:

    oracle.jpeg.encode(apply(oracle.jpeg.decode(j, TJPF_BGR, flags)), quality, TJPF_BGR, subsample, flags, tj_version)

with ``apply`` numpy's per-channel lookup on the BGR frame.  Whole JPEG byte strings are
compared, nothing less.  The table is three different permutations (a swapped channel fails);
the inputs cover every colour-pass layout (4:4:4, 4:2:2, 4:2:0, 4:4:0 and grayscale), sizes
that are not whole MCUs, and a 4:2:2 frame of more than one 15-MCU strip with an edge strip;
the outputs 4:2:2 and 4:2:0 (the one-row and two-row forms of the fused IDCT + colour kernel
and of the encoder's sample store).
"""
import numpy as np
import pytest

from oracle import jpeg as J
from vfilter import tables
from vfilter.jpeg import TJFLAG_FASTUPSAMPLE, TurboJPEG

pytestmark = pytest.mark.gpu


def _perm(seed):
    return np.random.default_rng(seed).permutation(256).astype(np.uint8)


T3 = tables.stack(_perm(12), _perm(13), _perm(14))
T3B = tables.stack(_perm(15), _perm(16), _perm(17))

# (input subsampling, width, height)
INPUTS = [(J.TJSAMP_422, 16, 8), (J.TJSAMP_422, 17, 13), (J.TJSAMP_422, 250, 130), (J.TJSAMP_420, 17, 13),
          (J.TJSAMP_420, 48, 34), (J.TJSAMP_444, 9, 9), (J.TJSAMP_440, 24, 20), (J.TJSAMP_GRAY, 33, 17)]
BIG = 2  # the 250 x 130 4:2:2 input


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def jpegs():
    return [J.encode(J.synthetic_scene(50 + i, h, w), 90, J.TJPF_BGR, ss) for i, (ss, w, h) in enumerate(INPUTS)]


def apply(img, table):
    """cv2.LUT(img, table) for a (256, 3) or (256,) table on a BGR frame."""
    t = np.asarray(table).reshape(256, -1)
    return np.stack([t[:, c % t.shape[1]][img[..., c]] for c in range(3)], axis=-1)


_want_cache = {}


def want(j, table, quality=85, subsample=J.TJSAMP_422, flags=0, tj_version=3):
    key = (j, np.asarray(table).tobytes(), quality, subsample, flags, tj_version)
    if key not in _want_cache:
        _want_cache[key] = J.encode(apply(J.decode(j, J.TJPF_BGR, flags), table), quality, J.TJPF_BGR, subsample,
                                    flags, tj_version)
    return _want_cache[key]


@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
@pytest.mark.parametrize("i", range(len(INPUTS)))
def test_each_input_layout_to_each_output_form(tj, jpegs, i, out_ss):
    j = jpegs[i]
    assert tj.lut(j, T3, jpeg_subsample=out_ss) == want(j, T3, subsample=out_ss), (INPUTS[i], out_ss)


@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
def test_mixed_batch(tj, jpegs, out_ss):
    got = tj.lut_batch(jpegs, T3, jpeg_subsample=out_ss)
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, T3, subsample=out_ss), (INPUTS[i], out_ss)


@pytest.mark.parametrize("switch", ["VF_JPEG_FUSE_IDCT", "VF_JPEG_FUSE"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
def test_unfused_forms_carry_the_table(tj, jpegs, monkeypatch, switch, out_ss):
    monkeypatch.setenv(switch, "0")
    assert tj.lut(jpegs[BIG], T3, jpeg_subsample=out_ss) == want(jpegs[BIG], T3, subsample=out_ss)
    got = tj.lut_batch(jpegs, T3, jpeg_subsample=out_ss)  # and every layout of the separate colour kernel
    for i, (g, j) in enumerate(zip(got, jpegs)):
        assert g == want(j, T3, subsample=out_ss), (switch, INPUTS[i], out_ss)


def test_fast_upsample_and_turbojpeg_2(tj, jpegs, vf_ctx):
    j = jpegs[BIG]
    assert tj.lut(j, T3, flags=TJFLAG_FASTUPSAMPLE) == want(j, T3, flags=TJFLAG_FASTUPSAMPLE)
    assert TurboJPEG(ctx=vf_ctx, tj_version=2).lut(j, T3) == want(j, T3, tj_version=2)
    assert tj.lut(j, T3, quality=60) == want(j, T3, quality=60)


def test_one_channel_table_goes_to_every_channel(tj, jpegs):
    g = tables.gamma(2.2)
    for j in (jpegs[BIG], jpegs[-1]):
        assert tj.lut(j, g) == want(j, g)
        assert tj.lut(j, g.reshape(256, 1)) == want(j, g)


def test_invert_table_gives_the_invert_path_bytes(tj, jpegs):
    for j in jpegs:
        assert tj.lut(j, tables.invert()) == tj.invert(j) == J.invert_jpeg(j)


def test_submit_then_result_equals_lut_batch(tj, jpegs):
    ticket = tj.lut_batch_submit(jpegs, T3)
    got = [bytes(v) for v in tj.invert_batch_result(ticket)]
    assert got == tj.lut_batch(jpegs, T3) == [want(j, T3) for j in jpegs]


def test_two_tickets_in_flight_keep_their_own_tables(tj, jpegs):
    ta = np.array(T3)
    t1 = tj.lut_batch_submit(jpegs, ta)
    ta[:] = 0  # the table was copied at submit
    t2 = tj.lut_batch_submit(jpegs, T3B)
    t3 = tj.invert_batch_submit(jpegs)
    assert [bytes(v) for v in tj.invert_batch_result(t2)] == [want(j, T3B) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t1)] == [want(j, T3) for j in jpegs]
    assert [bytes(v) for v in tj.invert_batch_result(t3)] == [J.invert_jpeg(j) for j in jpegs]


def test_bad_tables_are_refused(tj, jpegs):
    with pytest.raises(ValueError):
        tj.lut(jpegs[0], np.zeros((256, 2), np.uint8))
    with pytest.raises(ValueError):
        tj.lut_batch_submit(jpegs, np.zeros(256, np.int16))
    assert tj.lut(jpegs[0], T3) == want(jpegs[0], T3)


def test_lut_worker_jpeg_and_raw(jpegs):
    from vfilter.lut_worker import LutWorker
    kw = dict(install_signal_handlers=False, transport="tcp")
    j = jpegs[BIG]
    w = LutWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=True, table=T3, **kw)
    try:
        assert bytes(w(j)) == want(j, T3)
        res = w.process_batch([j, jpegs[0]], [None, None], [None, None])
        assert [bytes(r) for r in res] == [want(j, T3), want(jpegs[0], T3)]
        h = w.submit_batch([j, jpegs[3]], [None, None], [None, None])
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [want(j, T3), want(jpegs[3], T3)]
    finally:
        w.close()
    rng = np.random.default_rng(60)
    frames = [rng.integers(0, 256, (12, 10, 3), dtype=np.uint8) for _ in range(3)]
    w = LutWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, table=T3, **kw)
    try:
        assert bytes(w(frames[0].tobytes())) == apply(frames[0], T3).tobytes()
        out1 = np.empty(360, np.uint8)
        res = w.process_batch([f.tobytes() for f in frames], [None] * 3, [None, out1, None])
        assert res[1] is out1
        assert [bytes(r) for r in res] == [apply(f, T3).tobytes() for f in frames]
        h = w.submit_batch([f.tobytes() for f in frames], [None] * 3, [None] * 3)
        res, _ = w.poll_batch(h, True)
        assert [bytes(r) for r in res] == [apply(f, T3).tobytes() for f in frames]
        bad = w.process_batch([frames[0].tobytes(), bytes(16)], [None] * 2, [None] * 2)  # 16 B: not whole pixels
        assert bytes(bad[0]) == apply(frames[0], T3).tobytes() and isinstance(bad[1], Exception)
    finally:
        w.close()


def test_ring_batches_of_all_three_workers(jpegs):
    """``submit_ring_batch`` -> ``poll_batch`` on the "jpeg_ring" handle: JPEGs read from ring slots by
    address, results written into the slots' output halves.  A record outside the ring, a raw table or
    kernel worker and a worker with a delay all decline (None: the loop takes the per-frame views path)."""
    import _conv_ref as R
    from vfilter import shm, wire
    from vfilter.conv_worker import ConvWorker
    from vfilter.inverter import InverterWorker
    from vfilter.lut_worker import LutWorker
    from vfilter.worker import RingResults
    kern = R.kernel_set()["random3x5"]
    ins = [jpegs[BIG], jpegs[3], jpegs[-1]]  # 250 x 130 4:2:2, 17 x 13 4:2:0, 33 x 17 grey
    wants = {
        InverterWorker: [J.invert_jpeg(j) for j in ins],
        LutWorker: [want(j, T3) for j in ins],
        ConvWorker: [J.encode(R.filter2d(J.decode(j, J.TJPF_BGR), kern[0], kern[1], "reflect101"), 85, J.TJPF_BGR,
                              J.TJSAMP_422) for j in ins],
    }
    own = {InverterWorker: {}, LutWorker: {"table": T3}, ConvWorker: {"kernel": kern}}
    kw = dict(install_signal_handlers=False, transport="tcp")
    ring = shm.FrameRing(nslots=4, slot_bytes=65536)
    workers = []

    def make(cls, delay=0.0, use_jpeg=True):
        w = cls("127.0.0.1", 1, 1, delay, use_jpeg=use_jpeg, **own[cls], **kw)
        workers.append(w)
        w.on_ring_attached(ring)
        return w

    def done(w):
        workers.remove(w)
        w.close()  # also takes the ring's page-lock back, for the next worker's context

    try:
        cols = np.zeros(3, wire.COLS)
        for i, (slot, j) in enumerate(zip((0, 1, 3), ins)):
            assert len(j) <= ring.slot_bytes
            ring.in_view(slot, len(j))[:] = np.frombuffer(j, np.uint8)
            cols[i] = (i, len(j), slot, 0, (0, 0, 0, 0))
        for cls in (InverterWorker, LutWorker, ConvWorker):
            w = make(cls)
            for slot in (0, 1, 3):
                ring.out_view(slot, ring.slot_bytes)[:] = 0  # nothing left of the worker before
            h = w.submit_ring_batch(ring, cols)
            assert h is not None and h[0] == "jpeg_ring", cls
            res, _ = w.poll_batch(h, True)
            assert isinstance(res, RingResults) and not res.errors and not res.overflow, cls
            for i, wanted in enumerate(wants[cls]):
                assert int(res.nbytes[i]) == len(wanted), (cls, i)
                assert ring.out_view(int(cols["slot"][i]), int(res.nbytes[i])).tobytes() == wanted, (cls, i)
            for field, value in (("slot", 4), ("slot", -1), ("nbytes", ring.slot_bytes + 1)):
                bad = cols.copy()
                bad[field][1] = value
                assert w.submit_ring_batch(ring, bad) is None, (cls, field, value)
            done(w)
        for cls, delay, use_jpeg in ((LutWorker, 0.0, False), (ConvWorker, 0.0, False), (InverterWorker, 0.001, True),
                                     (LutWorker, 0.001, True), (ConvWorker, 0.001, True)):
            w = make(cls, delay, use_jpeg)
            assert w.submit_ring_batch(ring, cols) is None, (cls, delay, use_jpeg)
            done(w)
    finally:
        for w in workers:
            w.close()
        ring.close()


def test_invert_is_unchanged_after_lut_calls(tj, jpegs):
    j = jpegs[BIG]
    assert tj.lut(j, T3) == want(j, T3)
    assert tj.invert_batch([j]) == [J.invert_jpeg(j)]
    for ss in (J.TJSAMP_422, J.TJSAMP_420):
        assert tj.invert_batch(jpegs, jpeg_subsample=ss) == [J.invert_jpeg(x, jpeg_subsample=ss) for x in jpegs]
    assert np.array_equal(tj.decode(j), J.decode(j))  # a decode on a codec that last held a table
