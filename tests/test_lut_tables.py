"""The table filter's host side, without a GPU: the table convention (``vfilter.as_table``), the
builders of ``vfilter.tables``, and that the new entry points fail loudly without a device or a
context (there is no CPU fallback)."""
import os

import numpy as np
import pytest

import vfilter
from vfilter import _lib, tables

RNG = np.random.default_rng(20)


@pytest.mark.parametrize("shape", [(256,), (256, 1), (1, 256)])
def test_as_table_one_channel_shapes(shape):
    t = RNG.integers(0, 256, 256, dtype=np.uint8)
    planar, channels = vfilter.as_table(t.reshape(shape))
    assert channels == 1 and planar == t.tobytes()


@pytest.mark.parametrize("shape", [(256, 3), (256, 1, 3), (1, 256, 3)])
def test_as_table_three_channel_shapes_are_laid_out_planar(shape):
    t = RNG.integers(0, 256, (256, 3), dtype=np.uint8)
    planar, channels = vfilter.as_table(t.reshape(shape))
    assert channels == 3 and len(planar) == 768
    for c in range(3):
        for v in range(256):
            assert planar[c * 256 + v] == t[v, c]


def test_as_table_takes_a_non_contiguous_view():
    t = RNG.integers(0, 256, (3, 256), dtype=np.uint8)
    planar, channels = vfilter.as_table(t.T)  # (256, 3), strided
    assert channels == 3 and planar == t.tobytes()


@pytest.mark.parametrize("bad", [
    np.zeros(255, np.uint8), np.zeros(257, np.uint8), np.zeros((3, 256), np.uint8), np.zeros((256, 2), np.uint8),
    np.zeros((256, 4), np.uint8), np.zeros((2, 128), np.uint8), np.zeros((256, 3, 1), np.uint8), np.zeros(768, np.uint8),
    np.zeros(256, np.int8), np.zeros(256, np.uint16), np.zeros(256, np.float32), np.zeros((256, 3), np.int32),
])
def test_as_table_refuses_wrong_sizes_and_dtypes(bad):
    with pytest.raises(ValueError):
        vfilter.as_table(bad)


def test_builders():
    ar = np.arange(256)
    for t in (tables.identity(), tables.invert(), tables.gamma(2.2), tables.levels(1.3, -20), tables.threshold(100),
              tables.posterize(3)):
        assert t.shape == (256,) and t.dtype == np.uint8
    assert np.array_equal(tables.identity(), ar)
    assert np.array_equal(tables.invert(), 255 - ar)
    assert np.array_equal(tables.levels(1, 0), ar)
    assert tables.levels(2.5, 0)[101] == 252  # 252.5 rounds half to even
    assert tables.levels(2.5, 0)[102] == 255  # saturated
    assert tables.levels(2.5, 0)[1] == 2      # 2.5 -> 2
    assert tables.levels(1.5, 0)[1] == 2      # 1.5 -> 2
    assert np.array_equal(tables.levels(-1, 0), ar)  # the absolute value
    assert np.array_equal(tables.posterize(8), ar)
    assert np.array_equal(tables.posterize(1), np.where(ar >= 128, 128, 0))
    assert tables.threshold(127)[127] == 0 and tables.threshold(127)[128] == 255
    assert np.array_equal(tables.gamma(1.0), ar)
    g = tables.gamma(2.2)
    assert g[0] == 0 and g[255] == 255 and np.all(np.diff(g.astype(int)) >= 0) and g[64] > 64


def test_stack_is_the_bgr_table():
    b, g, r = tables.identity(), tables.invert(), tables.threshold(10)
    t = tables.stack(b, g, r)
    assert t.shape == (256, 3) and t.dtype == np.uint8
    planar, channels = vfilter.as_table(t)
    assert channels == 3 and planar == b.tobytes() + g.tobytes() + r.tobytes()
    with pytest.raises(ValueError):
        tables.stack(b, g, r.astype(np.int32))


def test_lut_refuses_bad_arguments_before_any_device_work():
    t3 = tables.stack(tables.identity(), tables.identity(), tables.identity())
    with pytest.raises(ValueError):
        vfilter.lut(np.zeros((4, 4), np.uint8), t3)          # 3-channel table, src.shape[-1] != 3
    with pytest.raises(ValueError):
        vfilter.lut(np.zeros((4, 4, 3), np.uint16), tables.identity())
    with pytest.raises(ValueError):
        vfilter.lut(np.zeros((4, 4, 3), np.uint8), np.zeros(100, np.uint8))
    with pytest.raises(ValueError):
        vfilter.lut_frames([bytes(16)], t3)                   # not whole pixels


def test_null_ctx_calls_fail_with_invalid():
    lib = _lib.load_library()
    t = tables.identity()
    assert lib.vf_lut_device(None, None, None, 10, t.ctypes.data, 1, None) == _lib.VF_E_INVALID
    assert b"ctx is NULL" in lib.vf_last_error(None)
    assert lib.vf_lut_frames_host(None, None, None, None, 0, t.ctypes.data, 1) == _lib.VF_E_INVALID
    assert lib.vf_jpeg_lut(None, None, None, 0, t.ctypes.data, 1, 85, 1, 0, None, None, None) == _lib.VF_E_INVALID
    assert lib.vf_jpeg_lut_submit(None, None, None, 1, t.ctypes.data, 1, 85, 1, 0, None) == _lib.VF_E_INVALID
    assert lib.vf_jpeg_bench_lut(None, None, None, 1, t.ctypes.data, 1, 85, 1, 0, 1, None, None) == _lib.VF_E_INVALID
    assert b"ctx is NULL" in lib.vf_last_error(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_fails_loudly():
    with pytest.raises(vfilter.VFilterError):
        vfilter.lut(np.zeros((4, 4, 3), np.uint8), tables.gamma(2.2), ctx=None)
    with pytest.raises(vfilter.VFilterError):
        vfilter.lut_frames([np.zeros(12, np.uint8)], tables.invert())
