"""The pointwise stream kernels under a capped grid: the table filter, the colour matrix, the histogram
and the level filter, chains of them, and the binary and invert kernels, each against the numpy
reference its own test file uses.  Every comparison is exact.

Every one of these kernels gives a workgroup whole tiles at a stride of ``gridDim.x`` tiles, the single
partial tile to whichever workgroup reaches it, and the head and tail bytes to workgroup 0; the
three-channel ones carry a channel phase from tile to tile, ``c = mod3_inc(c, stride % 3)``.  The grid's
cap is 32 workgroups per CU (8192; the histogram's own is 1024), so a frame below 128 MiB (16 MiB) never
runs that loop a second time.  ``vf_create`` reads ``VF_MAX_BLOCKS`` per context and the histogram takes
the smaller of that and its own cap, so the contexts here are capped at 1, 2, 3 and 5 workgroups: a few
hundred KiB then stride as a production frame does.  A tile is ``TILE`` = 256 lanes x 4 vectors x 16 B, for
the matrix ``MIX_TILE`` = 256 lanes x 2 units x 48 B; a stride of ``cap`` tiles of 1024 vectors moves the
phase by ``cap * 1024 % 3`` = 1, 2, 0 and 2:

    cap 1   one workgroup does everything, at the step of the histogram's production cap (1024 % 3)
    cap 2   the step of the production cap (8192 % 3)
    cap 3   step 0, where a missing advance would go unseen: nothing may depend on a nonzero step
    cap 5   uneven shares

Frames: A = 317 x 331 x 3 = 314,781 B, 19 whole tiles and a partial one (12 and a partial one of the
matrix's), which falls to workgroup 19 % cap = 0, 1, 1, 4; as one channel it is 317 x 993.  B = 256 x 256 x 3
= 196,608 B, exactly 12 tiles (8 of the matrix's): on an aligned buffer no partial tile, no head and no
tail.  Every frame has more than 2 x cap whole tiles under every cap, so some workgroup takes a third tile,
but B under the matrix at cap 5 (8 tiles), so the matrix also runs C = 352 x 256 x 3 = 270,336 B, exactly 11
of its tiles.  ``test_the_sizes_stride`` holds all of this arithmetic and needs no GPU: a later change of a
tile size fails it with a reason instead of leaving the GPU tests passing without a stride.

Contents: seeded random bytes; for the level filter random bytes in another range per channel, so that
the three tables differ; ``test_gpu_level.py``'s ``channel_constants`` (9, 130, 251), on which a phase slip
changes every byte of a histogram or a table lookup; and for the histogram a constant frame.

One more case runs on the session's context, at the histogram's real cap: 1025 tiles + 7 vectors + 6 B.
"""
import collections

import numpy as np
import pytest

import _chain_ref as CR
import _chain_ref_level as CL
import _level_ref as R
import _mix_ref as M
import vfilter
from vfilter import Level, Mix, colors, tables
from vfilter import kernels as K
from vfilter.filters import BINARY_OPS, Invert, Kernel, Table

gpu = pytest.mark.gpu

TILE = 16384      # bytes of a tile of the table, histogram, level, binary and invert kernels
MIX_TILE = 24576  # bytes of a tile of the colour matrix
CAPS = (1, 2, 3, 5)
A = (317, 331, 3)
B = (256, 256, 3)
C = (352, 256, 3)  # the matrix's B at cap 5
STREAM_OFFSETS = [(0, 0), (1, 1), (7, 7), (14, 14), (15, 15)]  # src and dst agree mod 16: the stream kernels
BYTEWISE = (3, 8)                                              # they differ: the bytewise kernels
PAD = 32  # the canary before and after a device destination, 0xEE


def _nbytes(shape):
    return shape[0] * shape[1] * shape[2]


def test_the_sizes_stride():
    assert (_nbytes(A), _nbytes(B), _nbytes(C)) == (314781, 196608, 270336)
    assert TILE == 256 * 4 * 16 and MIX_TILE == 256 * 2 * 48
    for cap in CAPS:
        for shape in (A, B):
            assert _nbytes(shape) // TILE > 2 * cap, (cap, shape)
        for shape in (A, C):
            assert _nbytes(shape) // MIX_TILE > 2 * cap, (cap, shape)
        # B has 8 tiles of the matrix: more than 2 x cap up to cap 3; at cap 5 three workgroups still take a
        # second tile, and C stands in for the third
        assert _nbytes(B) // MIX_TILE > (2 * cap if cap <= 3 else cap), cap
    for tile in (TILE, MIX_TILE):
        assert _nbytes(A) % tile != 0 and _nbytes(B) % tile == 0  # A has a partial tile, B none
    assert _nbytes(C) % MIX_TILE == 0
    # A keeps its 19 (12) whole tiles and its partial one at any offset from a 16-byte boundary, where up to
    # 15 bytes (15 pixels) go to the head
    assert (_nbytes(A) - 15) // TILE == 19 and 0 < (_nbytes(A) - 15) % TILE < TILE - 16
    assert (_nbytes(A) - 45) // MIX_TILE == 12 and 0 < (_nbytes(A) - 45) % MIX_TILE < MIX_TILE - 48
    assert [19 % cap for cap in CAPS] == [0, 1, 1, 4]  # the workgroup of A's partial tile
    assert [cap * (TILE // 16) % 3 for cap in CAPS] == [1, 2, 0, 2]
    assert {cap * (TILE // 16) % 3 for cap in CAPS} == {0, 1, 2}
    assert 1024 * (TILE // 16) % 3 == 1 and 8192 * (TILE // 16) % 3 == 2  # the production caps' steps: caps 1 and 2
    # the body's first byte takes every channel over the stream offsets
    assert {(16 - so) % 16 % 3 for so, _ in STREAM_OFFSETS} == {0, 1, 2}
    assert all(so == do for so, do in STREAM_OFFSETS) and BYTEWISE[0] != BYTEWISE[1]
    # the invert of three frames in one launch: cap / 3 + 1 workgroups a frame
    assert [cap // 3 + 1 for cap in CAPS] == [1, 1, 2, 2] and _nbytes(A) // TILE > 2 * 2
    # the host table case: 1 MiB pieces of a 3-channel frame start at channel 0, 1 and 2, 64 tiles each
    assert HOST_LUT_BYTES % 3 == 0 and [(k << 20) % 3 for k in range(3)] == [0, 1, 2]
    assert (1 << 20) // TILE == 64 > 2 * max(CAPS) and 2 << 20 < HOST_LUT_BYTES < 3 << 20
    assert (HOST_LUT_BYTES - (2 << 20)) // TILE > 2 * max(CAPS)


# -- frames and references, made once and never written to -------------------------------------------------------

def _perm(seed):
    return np.random.default_rng(seed).permutation(256).astype(np.uint8)


TABLES = {"perm1": _perm(1), "perm3": tables.stack(_perm(2), _perm(3), _perm(4))}
HOST_LUT_BYTES = 2400003
RULES = [("equalize", Level.equalize(), (R.EQUALIZE, 0, 0, (0, 0))),
         ("stretch0", Level.stretch(), (R.STRETCH, 0, 0, (0, 0))),
         ("stretch1pc", Level.stretch(0.01), (R.STRETCH, 0, 0, (655, 655))),
         ("stretch_lo_hi", Level.stretch((0.3, 0.002)), (R.STRETCH, 0, 0, (19661, 131)))]
MASKS = [((0, 2), True), ((1,), False)]  # the channels a level filter names, and link
CONTENTS = ["random", "random2", "ranges", "constant", "channel_constants"]
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
        _CACHE[key] = v
    return _CACHE[key]


def _frame(content, shape, c=3):
    """The bytes of ``shape`` (H x W x 3) with ``content``, as three channels or, ``c`` = 1, as H x 3 W."""
    def make():
        h, w, _ = shape
        rng = np.random.default_rng([h, w, CONTENTS.index(content)])
        if content == "random":
            a = rng.integers(0, 256, shape, dtype=np.uint8)
        elif content == "random2":
            a = rng.integers(0, 256, shape, dtype=np.uint8)[::-1].copy() // 2 + 17
        elif content == "ranges":  # every channel another range: three different level tables
            a = np.stack([rng.integers(30, 120, (h, w)), rng.integers(100, 250, (h, w)), rng.integers(0, 61, (h, w))],
                         axis=2).astype(np.uint8)
        elif content == "constant":
            a = np.full(shape, 200, np.uint8)
        else:
            assert content == "channel_constants"
            a = np.empty(shape, np.uint8)
            a[:, :, 0], a[:, :, 1], a[:, :, 2] = 9, 130, 251
        return a
    a = _once(("frame", content, shape), make)
    return a if c == 3 else a.reshape(shape[0], shape[1] * 3)


def _lut_ref(src, table, phase=0):
    """numpy's cv2.LUT over a flat frame whose byte 0 has channel ``phase`` (``tests/test_gpu_lut.py``'s)."""
    planar, channels = vfilter.as_table(table)
    t = np.frombuffer(planar, np.uint8).reshape(channels, 256)
    src = np.asarray(src).reshape(-1)
    if channels == 1:
        return t[0][src]
    return t[(np.arange(src.size) + phase) % 3, src]


def _lut_want(content, shape, name):
    return _once(("lut", content, shape, name), lambda: _lut_ref(_frame(content, shape), TABLES[name]))


def _matrices():
    out = dict(M.matrix_set())
    v = colors.sepia()
    out["colors.sepia"] = (v.matrix.astype(np.int64), v.shift) if isinstance(v, Mix) else (np.asarray(v[0], np.int64), v[1])
    return out


MATRICES = _matrices()
# shift 0 (nothing to round), half up and half even; negative weights; one that saturates at both ends
MIX_FORMS = [("shift0_offsets", "half_even"), ("all_negative_row", "half_up"), ("sum_65536_shift_16", "half_even"),
             ("colors.sepia", "half_even")]
CODE = {"half_even": 0, "half_up": 1}


def _mix_want(content, shape, name, rounding):
    return _once(("mix", content, shape, name, rounding),
                 lambda: M.mix(_frame(content, shape), *MATRICES[name], rounding))


def _hist_want(content, shape, c):
    return _once(("hist", content, shape, c), lambda: R.hist(_frame(content, shape, c)))


def _level_want(content, shape, c, rule, mask=0, link=0, clips=(0, 0)):
    return _once(("level", content, shape, c, rule, mask, link, clips),
                 lambda: R.level(_frame(content, shape, c), rule, mask, link, clips))


# -- capped contexts and device buffers -----------------------------------------------------------------------------

Capped = collections.namedtuple("Capped", "ctx cap")


@pytest.fixture(scope="module", params=CAPS, ids=lambda cap: "cap%d" % cap)
def capped(request):
    """A context whose stream kernels run on at most ``cap`` workgroups.  The cap is read in ``vf_create``, so
    the environment is restored as soon as the context exists."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VF_MAX_BLOCKS", str(request.param))
        ctx = vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1)
    try:
        yield Capped(ctx, request.param)
    finally:
        ctx.close()


class _Dev:
    """``count`` device buffers of ``n`` bytes between canaries, with room for an offset below 16."""

    def __init__(self, ctx, n, count=2):
        self.ctx, self.size = ctx, n + 2 * PAD + 16
        self.bufs = [ctx.alloc_device(self.size) for _ in range(count)]
        assert all(p % 16 == 0 for p in self.bufs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.sync()
        for p in self.bufs:
            self.ctx.free_device(p)

    def at(self, i, off):
        return self.bufs[i] + PAD + off

    def put(self, i, off, data):
        """Buffer i all canary, then ``data`` at ``off`` from a 16-byte boundary; its device address."""
        self.ctx.memset_device(self.bufs[i], 0xEE, self.size)
        self.ctx.sync()
        self.ctx.upload(self.at(i, off), data, data.nbytes)
        return self.at(i, off)

    def clear(self, i):
        self.ctx.memset_device(self.bufs[i], 0xEE, self.size)
        self.ctx.sync()

    def get(self, i, off, n, what):
        """The n bytes at ``off`` of buffer i, after checking the canaries on both sides."""
        self.ctx.sync()
        got = np.empty(self.size, np.uint8)
        self.ctx.download(got, self.bufs[i], self.size)
        self.ctx.sync()
        lo = PAD + off
        assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE), ("canary", what)
        return got[lo:lo + n]

    def run(self, src, so, do, launch, what):
        """``launch(dsrc, ddst)`` from buffer 0 at offset ``so`` into buffer 1 at ``do``."""
        s = self.put(0, so, src)
        self.clear(1)
        launch(s, self.at(1, do))
        return self.get(1, do, src.nbytes, what)

    def run_in_place(self, src, off, launch, what):
        s = self.put(0, off, src)
        launch(s, s)
        return self.get(0, off, src.nbytes, what)


def _where(got, want):
    return np.argwhere(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[:5].reshape(-1).tolist()


def _same(got, want, what):
    assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)), (what, _where(got, want))


# -- 1. the table filter ------------------------------------------------------------------------------------------------

@gpu
def test_table(capped):
    ctx, cap = capped
    n = _nbytes(A)
    with _Dev(ctx, n) as dev:
        for name in ("perm1", "perm3"):
            planar, channels = vfilter.as_table(TABLES[name])

            def launch(s, d, nb=n):
                ctx.lut_device(s, d, nb, planar, channels)

            for content in ("random", "channel_constants"):
                src, want = _frame(content, A).reshape(-1), _lut_want(content, A, name)
                for so, do in STREAM_OFFSETS + [BYTEWISE]:
                    _same(dev.run(src, so, do, launch, (cap, name, content, so, do)), want, (cap, name, content, so, do))
                for off in (0, 7):
                    _same(dev.run_in_place(src, off, launch, (cap, name, content, off)), want,
                          (cap, name, content, off, "in place"))
            src, nb = _frame("random", B).reshape(-1), _nbytes(B)  # whole tiles only
            _same(dev.run(src, 0, 0, lambda s, d: launch(s, d, nb), (cap, name, "B")), _lut_want("random", B, name),
                  (cap, name, "B"))
    # the host path: a frame of 2.3 MiB in 1 MiB of staging is cut mid-pixel into pieces that start at channels
    # 0, 1 and 2, and each piece strides
    big = _once(("host_lut",), lambda: np.random.default_rng(77).integers(0, 256, HOST_LUT_BYTES, dtype=np.uint8))
    for name in ("perm1", "perm3"):
        got = vfilter.lut_frames([big], TABLES[name], ctx=ctx)[0]
        _same(got, _once(("host_lut", name), lambda: _lut_ref(big, TABLES[name])), (cap, name, "host"))


# -- 2. the colour matrix -----------------------------------------------------------------------------------------------

@gpu
def test_colour_matrix(capped, monkeypatch):
    ctx, cap = capped
    assert ctx.mix_tile_bytes() == MIX_TILE
    with _Dev(ctx, _nbytes(A)) as dev:
        for form in (None, "stride"):
            if form:
                monkeypatch.setenv("VF_MIX_FORM", form)  # read per call
            else:
                monkeypatch.delenv("VF_MIX_FORM", raising=False)
            for name, rounding in MIX_FORMS:
                m, s = MATRICES[name]
                m32 = m.astype(np.int32)

                def launch(src, dst, nb):
                    ctx.mix_device(src, dst, nb, m32, s, CODE[rounding])

                src, want, n = _frame("random", A).reshape(-1), _mix_want("random", A, name, rounding), _nbytes(A)
                for so, do in [(3, 0), (0, 5), (8, 15), (0, 0)]:  # src off dst's 16-byte grid but for the last
                    what = (cap, form, name, rounding, so, do)
                    _same(dev.run(src, so, do, lambda a, b: launch(a, b, n), what), want, what)
                _same(dev.run_in_place(src, 5, lambda a, b: launch(a, b, n), (cap, form, name, "A in place")), want,
                      (cap, form, name, rounding, "A in place"))
                for shape in (B, C):  # whole tiles only, in place
                    src, nb = _frame("random", shape).reshape(-1), _nbytes(shape)
                    what = (cap, form, name, rounding, shape, "in place")
                    _same(dev.run_in_place(src, 0, lambda a, b: launch(a, b, nb), what),
                          _mix_want("random", shape, name, rounding), what)
                # and through the host path
                for content, shape in (("random", A), ("channel_constants", A), ("random", B)):
                    img = _frame(content, shape)
                    what = (cap, form, name, rounding, content, shape, "transform")
                    _same(vfilter.transform(img, (m, s), rounding=rounding, ctx=ctx), _mix_want(content, shape, name, rounding),
                          what)
                buf = _frame("random", A).copy()
                assert vfilter.transform(buf, (m, s), dst=buf, rounding=rounding, ctx=ctx) is buf
                _same(buf, _mix_want("random", A, name, rounding), (cap, form, name, rounding, "transform in place"))


# -- 3. the histogram ---------------------------------------------------------------------------------------------------

def _hist_device(ctx, dev, dh, src, off, c):
    got = np.empty((c, 256), np.uint32)
    ctx.hist_device(dev.put(0, off, src), src.nbytes, c, dh)
    ctx.sync()
    ctx.download(got, dh, c * 1024)
    ctx.sync()
    return got


@gpu
def test_histogram(capped):
    ctx, cap = capped
    n = _nbytes(A)
    store = np.empty(n + 64, np.uint8)
    base = (-store.ctypes.data) % 16
    with _Dev(ctx, n, 1) as dev:
        dh = ctx.alloc_device(3 * 1024)
        try:
            for c in (1, 3):
                for content in ("random", "channel_constants"):
                    img = _frame(content, A, c)
                    want = _hist_want(content, A, c)
                    assert want.sum(axis=1).tolist() == [n // c] * c
                    for off in range(16):
                        got = _hist_device(ctx, dev, dh, img.reshape(-1), off, c)
                        _same(got, want, (cap, c, content, off, "device"))
                        assert got.sum(axis=1).tolist() == [n // c] * c, (cap, c, content, off)
                        host = store[base + off:base + off + n]  # calc_hist keeps the caller's offset in its staging
                        assert host.ctypes.data % 16 == off
                        host[:] = img.reshape(-1)
                        got = vfilter.calc_hist(host.reshape(img.shape), ctx=ctx)
                        assert got.dtype == np.uint32 and got.shape == (c, 256)
                        _same(got, want, (cap, c, content, off, "host"))
                img = _frame("random", B, c)  # whole tiles only
                _same(_hist_device(ctx, dev, dh, img.reshape(-1), 0, c), _hist_want("random", B, c), (cap, c, "B device"))
                _same(vfilter.calc_hist(img, ctx=ctx), _hist_want("random", B, c), (cap, c, "B host"))
                # a constant frame: under cap 1 one workgroup counts all 314,781 bytes into one bin a channel
                img = _frame("constant", A, c)
                for got in (_hist_device(ctx, dev, dh, img.reshape(-1), 0, c), _hist_device(ctx, dev, dh, img.reshape(-1), 9, c),
                            vfilter.calc_hist(img, ctx=ctx)):
                    _same(got, _hist_want("constant", A, c), (cap, c, "constant"))
                    assert got[:, 200].tolist() == [n // c] * c and int(got.sum()) == n
        finally:
            ctx.sync()
            ctx.free_device(dh)


# -- 4. the level filter ------------------------------------------------------------------------------------------------

def _level_cases(c):
    """(name, Level, the reference's arguments): the four rules, and on three channels the mask and link pairs."""
    cases = list(RULES)
    if c == 3:
        for chans, link in MASKS:
            mask = sum(1 << k for k in chans)
            cases.append(("equalize%s" % (chans,), Level.equalize(chans, link), (R.EQUALIZE, mask, int(link), (0, 0))))
            cases.append(("stretch1pc%s" % (chans,), Level.stretch(0.01, chans, link), (R.STRETCH, mask, int(link), (655, 655))))
    return cases


@gpu
def test_level(capped):
    ctx, cap = capped
    h, w, _ = A
    n = _nbytes(A)
    with _Dev(ctx, n) as dev:
        for c in (1, 3):
            wc = w * 3 // c  # A as one channel is 317 x 993
            for name, lv, (rule, mask, link, clips) in _level_cases(c):
                assert lv.args == (rule, mask, link) + clips, name

                def launch(s, d, rule=rule, mask=mask, link=link, clips=clips):
                    ctx.level_device(s, d, wc, h, c, rule, mask, link, *clips)

                img, want = _frame("ranges", A, c), _level_want("ranges", A, c, rule, mask, link, clips)
                for so, do in [(0, 0), (7, 7), BYTEWISE]:
                    what = (cap, c, name, so, do)
                    _same(dev.run(img.reshape(-1), so, do, launch, what), want, what)
                _same(dev.run_in_place(img.reshape(-1), 7, launch, (cap, c, name, "in place")), want, (cap, c, name, "in place"))
                got = vfilter.level_frames([img], lv, ctx=ctx)[0]  # the host path
                assert got.shape == img.shape
                _same(got, want, (cap, c, name, "level_frames"))
            for content, shape in (("channel_constants", A), ("random", A), ("ranges", B)):
                img = _frame(content, shape, c)
                want = _level_want(content, shape, c, R.EQUALIZE)
                if content == "channel_constants" and c == 3:
                    assert np.array_equal(want, img)  # a constant channel stays; a slipped histogram would move it
                _same(vfilter.equalize_hist(img, ctx=ctx), want, (cap, c, content, shape, "equalize_hist"))
                nb = img.nbytes
                got = dev.run(img.reshape(-1), 0, 0,
                              lambda s, d: ctx.level_device(s, d, shape[1] * 3 // c, shape[0], c, R.STRETCH, 0, 0, 655, 655),
                              (cap, c, content, shape))
                assert got.size == nb
                _same(got, _level_want(content, shape, c, R.STRETCH, 0, 0, (655, 655)), (cap, c, content, shape, "device"))
            # three calls back to back on one stream, frames a, b, a: stale histogram words of b would change
            # the last table
            a, b = _frame("ranges", A, c).reshape(-1), _frame("random2", A, c).reshape(-1)
            dev.clear(1)
            for img in (a, b, a):
                ctx.upload(dev.at(0, 0), img, n)
                ctx.level_device(dev.at(0, 0), dev.at(1, 0), wc, h, c, R.STRETCH, 0, int(c == 3), 655, 655)
            _same(dev.get(1, 0, n, (cap, c, "a, b, a")), _level_want("ranges", A, c, R.STRETCH, 0, int(c == 3), (655, 655)),
                  (cap, c, "a, b, a"))


# -- 5. chains ----------------------------------------------------------------------------------------------------------

def _chain_programs():
    m, s = MATRICES["all_negative_row"]
    sharpen = K.sharpen()
    t3 = TABLES["perm3"]
    table, mix, level, invert = ("table", t3), ("mix", m, s, "half_even"), ("level", R.EQUALIZE, 0, 0, (0, 0)), ("table", CR.INVERT)
    conv = ("conv", np.asarray(sharpen[0]), sharpen[1], "reflect101")
    steps = {"table": Table(t3), "mix": Mix((m, s), "half_even"), "level": Level.equalize(), "invert": Invert(),
             "conv": Kernel(sharpen)}
    out = {}
    for name, order in (("pointwise", ("table", "mix", "level", "invert")), ("with_conv", ("table", "conv", "mix", "level", "invert"))):
        refs = dict(table=table, mix=mix, level=level, invert=invert, conv=conv)
        prog = [(refs[k][0], i) + tuple(refs[k][1:]) for i, k in enumerate(order)]
        out[name] = ([steps[k] for k in order], prog)
    return out


@gpu
def test_chain(capped):
    """The table, matrix and level steps of a chain take the context's cap; the neighbourhood kernels launch one
    workgroup a tile, take no cap and are not disturbed by it."""
    ctx, cap = capped
    img = _frame("random", A)
    for name, (steps, prog) in _chain_programs().items():
        want = _once(("chain", name), lambda: CL.run(img, prog))
        _same(vfilter.chain(img, steps, ctx=ctx), want, (cap, name))
        buf = img.copy()
        assert vfilter.chain(buf, steps, dst=buf, ctx=ctx) is buf
        _same(buf, want, (cap, name, "in place"))


# -- 6. binary and invert -----------------------------------------------------------------------------------------------

@gpu
def test_binary_and_invert(capped):
    ctx, cap = capped
    n = _nbytes(A)
    a, b = _frame("random", A).reshape(-1), _frame("random2", A).reshape(-1)
    absdiff = np.abs(a.astype(np.int32) - b.astype(np.int32)).astype(np.uint8)
    with _Dev(ctx, n, 3) as dev:
        for oa, ob, od in [(5, 12, 0), (5, 12, 12)]:
            da, db = dev.put(0, oa, a), dev.put(1, ob, b)
            dev.clear(2)
            ctx.binary_device(da, db, dev.at(2, od), n, BINARY_OPS["absdiff"])
            _same(dev.get(2, od, n, (cap, "absdiff", od)), absdiff, (cap, "absdiff", oa, ob, od))
        got = dev.run(a, 5, 12, lambda s, d: ctx.invert_device(s, d, n), (cap, "invert"))  # the shift kernel
        _same(got, ~a, (cap, "invert", 5, 12))
        _same(dev.run(a, 9, 9, lambda s, d: ctx.invert_device(s, d, n), (cap, "invert")), ~a, (cap, "invert", 9, 9))
    # three frames in one launch: cap / 3 + 1 = 1, 1, 2, 2 workgroups a frame
    frames = [a, b, _frame("channel_constants", A).reshape(-1)]
    offs = [(0, 0), (3, 3), (5, 12)]
    with _Dev(ctx, n, 6) as dev:
        tabs = [ctx.alloc_device(64) for _ in range(3)]
        try:
            for i, (f, (so, _)) in enumerate(zip(frames, offs)):
                dev.put(i, so, f)
                dev.clear(3 + i)
            sp = np.array([dev.at(i, so) for i, (so, _) in enumerate(offs)], np.uint64)
            dp = np.array([dev.at(3 + i, do) for i, (_, do) in enumerate(offs)], np.uint64)
            nb = np.array([n] * 3, np.uint64)
            for t, arr in zip(tabs, (sp, dp, nb)):
                ctx.upload(t, arr, arr.nbytes)
            ctx.invert_device_frames(tabs[0], tabs[1], tabs[2], 3, 3 * n)
            for i, (f, (_, do)) in enumerate(zip(frames, offs)):
                _same(dev.get(3 + i, do, n, (cap, "frames", i)), ~f, (cap, "frames", i))
        finally:
            ctx.sync()
            for t in tabs:
                ctx.free_device(t)


# -- the histogram's own cap, on the session's context --------------------------------------------------------------------

@gpu
def test_one_tile_more_than_the_histograms_cap(vf_ctx):
    """1025 tiles + 7 vectors + 6 B: the smallest frame that strides under ``kHistMaxBlocks`` = 1024, which no
    environment cap can show to be right itself.  The level filter's apply pass runs one tile a workgroup here."""
    n = 1025 * TILE + 7 * 16 + 6
    assert n == 16793718 and n % 3 == 0 and n > 1024 * 16384
    data = np.random.default_rng(1025).integers(0, 256, n, dtype=np.uint8) // 2  # another range a channel
    data += np.tile(np.array([20, 50, 90], np.uint8), n // 3)
    got, hist = np.empty(n, np.uint8), np.empty(3 * 256, np.uint32)
    dsrc, ddst, dh = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n), vf_ctx.alloc_device(3 * 1024)
    try:
        vf_ctx.upload(dsrc, data, n)
        for c in (3, 1):
            h = 2
            w = n // c // h
            assert w * h * c == n
            img = data.reshape(h, w, 3) if c == 3 else data.reshape(h, w)
            vf_ctx.hist_device(dsrc, n, c, dh)
            vf_ctx.level_device(dsrc, ddst, w, h, c, R.STRETCH, 0, 0, 655, 655)
            vf_ctx.sync()
            vf_ctx.download(hist, dh, c * 1024)
            vf_ctx.download(got, ddst, n)
            vf_ctx.sync()
            _same(hist[:c * 256], R.hist(img), (c, "hist"))
            _same(got, R.level(img, R.STRETCH, 0, 0, (655, 655)), (c, "level"))
    finally:
        vf_ctx.sync()
        for p in (dsrc, ddst, dh):
            vf_ctx.free_device(p)
