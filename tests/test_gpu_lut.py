"""The 256-entry table filter on raw frames (``vf_lut_frames_host``, ``vf_lut_device``,
``vfilter.lut``) against numpy: ``table.reshape(C, 256)[channel_of_byte, src]``.  Every
comparison is exact.

One tile of the kernel is 256 lanes x 4 vectors x 16 B = 16 KiB, so the sizes sit around 16 B
(head / body / tail), around one tile (the partial tile) and past several (more than one
workgroup); the alignments cover every offset mod 16 and source and destination that disagree
(the bytewise kernel); the device case has one more tile than the grid's cap, so the grid
strides; the mixed batch has a frame larger than its context's staging, so it is cut mid-pixel.
The three-channel table is three different permutations: a swapped channel or a slipped phase
cannot pass.
"""
import ctypes

import numpy as np
import pytest

import vfilter
from vfilter import _lib, tables

pytestmark = pytest.mark.gpu

TILE = 256 * 4 * 16
SIZES3 = [0, 3, 15, 18, 48, 51, (TILE - 1) // 3 * 3, TILE + 2, 3 * TILE + 21]
SIZES1 = SIZES3 + [1, 2, 16, 17]


def _perm(seed):
    return np.random.default_rng(seed).permutation(256).astype(np.uint8)


TABLES = {
    "identity": tables.identity(),
    "invert": tables.invert(),
    "perm1": _perm(1),
    "perm3": tables.stack(_perm(2), _perm(3), _perm(4)),
}


def _ref(src, table, phase=0):
    """numpy's cv2.LUT over a flat frame whose byte 0 has channel ``phase``."""
    planar, channels = vfilter.as_table(table)
    t = np.frombuffer(planar, np.uint8).reshape(channels, 256)
    src = np.asarray(src).reshape(-1)
    if channels == 1:
        return t[0][src]
    return t[(np.arange(src.size) + phase) % 3, src]


def _data(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _at_offset(n, a):
    """An n-byte uint8 view whose address is ``a`` mod 16 (its base keeps it alive)."""
    base = np.zeros(n + 32, np.uint8)
    off = (a - base.ctypes.data) % 16
    v = base[off:off + n]
    assert v.ctypes.data % 16 == a
    return v


@pytest.mark.parametrize("name", list(TABLES))
def test_sizes_around_a_vector_and_a_tile(vf_ctx, name):
    table = TABLES[name]
    channels = vfilter.as_table(table)[1]
    for n in (SIZES3 if channels == 3 else SIZES1):
        src = _data(n, n)
        keep = src.copy()
        got = vfilter.lut_frames([src], table, ctx=vf_ctx)[0]
        assert np.array_equal(src, keep)
        if name == "identity":
            assert np.array_equal(got, src), n
        assert np.array_equal(got, _ref(src, table)), (name, n)
        if name == "invert" and n:  # the existing kernel, on the same input
            assert np.array_equal(got, vfilter.bitwise_not(src, ctx=vf_ctx)), n


@pytest.mark.parametrize("name", ["perm1", "perm3"])
def test_every_common_alignment(vf_ctx, name):
    table = TABLES[name]
    n = 48 * 1024 + 21
    data = _data(7, n)
    want = _ref(data, table)
    for a in range(16):
        src, dst = _at_offset(n, a), _at_offset(n, a)
        src[:] = data
        vfilter.lut_frames([src], table, outs=[dst], ctx=vf_ctx)
        assert np.array_equal(dst, want), a


@pytest.mark.parametrize("name", ["perm1", "perm3"])
@pytest.mark.parametrize("sa,da", [(1, 0), (0, 5), (7, 12)])
def test_source_and_destination_misaligned_to_each_other(vf_ctx, name, sa, da):
    table = TABLES[name]
    n = 48 * 1024 + 21
    src, dst = _at_offset(n, sa), _at_offset(n, da)
    src[:] = _data(8, n)
    vfilter.lut_frames([src], table, outs=[dst], ctx=vf_ctx)
    assert np.array_equal(dst, _ref(src, table))


@pytest.mark.parametrize("name", ["perm1", "perm3"])
def test_in_place(vf_ctx, name):
    table = TABLES[name]
    buf = _data(9, 3 * TILE + 21)
    want = _ref(buf, table)
    out = vfilter.lut_frames([buf], table, outs=[buf], ctx=vf_ctx)[0]
    assert out is buf and np.array_equal(buf, want)
    img = _data(11, 21 * 17 * 3).reshape(21, 17, 3)  # and cv2.LUT(src, lut, dst) with dst = src
    want = _ref(img, table).reshape(img.shape)
    assert vfilter.lut(img, table, dst=img, ctx=vf_ctx) is img and np.array_equal(img, want)


def test_lut_is_cv2_lut_on_an_image(vf_ctx):
    img = _data(10, 37 * 53 * 3).reshape(37, 53, 3)
    t3 = TABLES["perm3"]
    got = vfilter.lut(img, t3, ctx=vf_ctx)
    assert got.shape == img.shape and got.dtype == np.uint8
    for c in range(3):
        assert np.array_equal(got[..., c], t3[:, c][img[..., c]])
    for shape in ((256, 1, 3), (1, 256, 3)):
        assert np.array_equal(vfilter.lut(img, t3.reshape(shape), ctx=vf_ctx), got)
    g = tables.gamma(2.2)
    assert np.array_equal(vfilter.lut(img, g, ctx=vf_ctx), g[img])
    assert np.array_equal(vfilter.lut(img[..., 0], g.reshape(1, 256), ctx=vf_ctx), g[img[..., 0]])  # strided view


@pytest.mark.parametrize("name", ["perm1", "perm3"])
def test_mixed_batch_with_a_frame_larger_than_the_staging(name):
    """max_frame_bytes = 1 MiB: the 1080p frame takes six fills, cut at 1 MiB (= 1 mod 3) each."""
    table = TABLES[name]
    sizes = [0, 3, 49152, 300, 6220800]
    frames = [_data(20 + i, n) for i, n in enumerate(sizes)]
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        got = vfilter.lut_frames(frames, table, ctx=ctx)
    for f, g in zip(frames, got):
        assert np.array_equal(g, _ref(f, table)), f.size


def test_device_resident_grid_stride(vf_ctx):
    """8193 tiles + 7 vectors + 5 B: one more tile than the grid's cap of 8192 workgroups."""
    n = 8193 * TILE + 7 * 16 + 5
    assert n % 3 == 0
    t3 = TABLES["perm3"]
    planar, channels = vfilter.as_table(t3)
    src = _data(30, n)
    got = np.empty_like(src)
    dsrc, ddst = vf_ctx.alloc_device(n), vf_ctx.alloc_device(n)
    try:
        vf_ctx.upload(dsrc, src, n)
        vf_ctx.lut_device(dsrc, ddst, n, planar, channels)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    px, gx = src.reshape(-1, 3), got.reshape(-1, 3)
    for c in range(3):
        assert np.array_equal(gx[:, c], t3[:, c][px[:, c]]), c


@pytest.mark.parametrize("so,do", [(0, 0), (3, 3), (9, 9), (1, 0), (0, 5), (7, 12)])
def test_device_pointers_at_any_alignment(vf_ctx, so, do):
    n = TILE + 16 * 5 + 9  # 16473 = 3 * 5491
    assert n % 3 == 0
    t3 = TABLES["perm3"]
    planar, channels = vfilter.as_table(t3)
    src = _data(31, n)
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, src, n)
        vf_ctx.lut_device(dsrc + so, ddst + do, n, planar, channels)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(dsrc)
        vf_ctx.free_device(ddst)
    assert np.array_equal(got[do:do + n], _ref(src, t3))
    assert np.all(got[:do] == 0xEE) and np.all(got[do + n:] == 0xEE)  # nothing outside the range


def test_errors_leave_the_context_usable(vf_ctx):
    lib = _lib.load_library()
    t1, t3 = vfilter.as_table(TABLES["perm1"])[0], vfilter.as_table(TABLES["perm3"])[0]
    src = _data(40, 16)
    dst = np.empty_like(src)
    probe = _data(41, 300)

    def still_works():
        assert np.array_equal(vfilter.lut_frames([probe], TABLES["perm3"], ctx=vf_ctx)[0], _ref(probe, TABLES["perm3"]))

    with pytest.raises(vfilter.VFilterError) as ei:  # 16 bytes are not whole 3-channel pixels
        vf_ctx.lut_frames_host([src], [dst], [16], t3, 3)
    assert ei.value.status == _lib.VF_E_INVALID
    still_works()
    sa, da, na = (ctypes.c_void_p * 1)(src.ctypes.data), (ctypes.c_void_p * 1)(dst.ctypes.data), (ctypes.c_size_t * 1)(15)
    tb = np.frombuffer(t3, np.uint8)
    assert lib.vf_lut_frames_host(vf_ctx.handle, sa, da, na, 1, tb.ctypes.data, 2) == _lib.VF_E_INVALID
    assert b"channels" in lib.vf_last_error(None)
    still_works()
    assert lib.vf_lut_frames_host(vf_ctx.handle, sa, da, na, 1, None, 1) == _lib.VF_E_INVALID
    assert b"table is NULL" in lib.vf_last_error(None)
    still_works()
    d = vf_ctx.alloc_device(64)
    try:
        assert lib.vf_lut_device(vf_ctx.handle, d, d, 16, tb.ctypes.data, 3, None) == _lib.VF_E_INVALID
        assert lib.vf_lut_device(vf_ctx.handle, d, d, 15, tb.ctypes.data, 2, None) == _lib.VF_E_INVALID
        assert lib.vf_lut_device(vf_ctx.handle, d, d, 15, None, 3, None) == _lib.VF_E_INVALID
    finally:
        vf_ctx.free_device(d)
    still_works()
    assert np.array_equal(vfilter.lut_frames([src], np.frombuffer(t1, np.uint8), ctx=vf_ctx)[0], _ref(src, TABLES["perm1"]))
