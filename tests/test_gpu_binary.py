"""The two-input per-byte kernel (``vf_binary_device``, csrc/vf_binary.hip) against numpy.  Every
comparison is exact.

``dst[i] = op(a[i], b[i])`` for ``subtract`` (max(a - b, 0)), ``add`` (min(a + b, 255)), ``absdiff``,
``min`` and ``max``.  The truth table covers every byte pair.  One tile of the kernel is 256 lanes x 4
vectors x 16 B = 16 KiB and the 16-B grid is the destination's, so the lengths sit around a vector
(head / body / tail), around 4096 and past several tiles, and the three pointers take offsets mod
16 that agree and that differ; a context with a grid of two workgroups makes the grid stride.
"""
import numpy as np
import pytest

import vfilter
from vfilter import _lib
from vfilter.filters import BINARY_OPS

pytestmark = pytest.mark.gpu

OPS = ["subtract", "add", "absdiff", "min", "max"]
LENGTHS = [1, 15, 16, 17, 4095, 4096, 4097, 300001]
ALIGNMENTS = [(0, 0, 0), (1, 5, 11), (15, 8, 3)]
PAD = 16  # the canary before and after dst


def _ref(op, a, b):
    x, y = a.astype(np.int32), b.astype(np.int32)
    r = {"subtract": np.maximum(x - y, 0), "add": np.minimum(x + y, 255), "absdiff": np.abs(x - y),
         "min": np.minimum(x, y), "max": np.maximum(x, y)}[op]
    return r.astype(np.uint8)


class _Dev:
    """Three device buffers of ``cap`` bytes (+ slack for the offsets and the canaries)."""

    def __init__(self, ctx, cap):
        self.ctx, self.size = ctx, cap + 2 * PAD + 32
        self.bufs = [ctx.alloc_device(self.size) for _ in range(3)]
        assert all(p % 16 == 0 for p in self.bufs)

    def close(self):
        for p in self.bufs:
            self.ctx.free_device(p)

    def run(self, op, a, b, offs=(0, 0, 0), dst_is=None):
        """op(a, b) with the three pointers at offs mod 16; dst_is "a" / "b": in place.  Returns the
        result after checking the canaries around dst."""
        ctx, n = self.ctx, a.size
        da, db, dd = (p + PAD + o for p, o in zip(self.bufs, offs))
        if dst_is == "a":
            dd = da
        elif dst_is == "b":
            dd = db
        base = {"a": self.bufs[0], "b": self.bufs[1]}.get(dst_is, self.bufs[2])
        ctx.memset_device(base, 0xEE, self.size)
        ctx.sync()
        ctx.upload(da, a, n)
        ctx.upload(db, b, n)
        ctx.binary_device(da, db, dd, n, BINARY_OPS[op])
        ctx.sync()
        got = np.empty(self.size, np.uint8)
        ctx.download(got, base, self.size)
        ctx.sync()
        lo = dd - base
        assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE), (op, n, offs, dst_is)
        return got[lo:lo + n]


@pytest.fixture(scope="module")
def dev(vf_ctx):
    d = _Dev(vf_ctx, max(LENGTHS))
    yield d
    d.close()


@pytest.mark.parametrize("op", OPS)
def test_every_byte_pair(dev, op):
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    assert a.size == 65536
    got = dev.run(op, a, b)
    want = _ref(op, a, b)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the definitions, spelt out on a few pairs: a = 3, b = 250 and the reverse
    i, j = 3 * 256 + 250, 250 * 256 + 3
    assert (int(want[i]), int(want[j])) == {"subtract": (0, 247), "add": (253, 253), "absdiff": (247, 247),
                                            "min": (3, 3), "max": (250, 250)}[op]
    assert int(_ref("add", a, b)[200 * 256 + 100]) == 255


@pytest.mark.parametrize("offs", ALIGNMENTS)
@pytest.mark.parametrize("op", OPS)
def test_lengths_and_alignments(dev, op, offs):
    rng = np.random.default_rng(sum(offs) + len(op))
    for n in LENGTHS:
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        got = dev.run(op, a, b, offs)
        assert np.array_equal(got, _ref(op, a, b)), (op, n, offs)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("op", OPS)
def test_in_place_over_either_operand(dev, op, which):
    rng = np.random.default_rng(17)
    for n, offs in [(17, (0, 0, 0)), (4097, (3, 3, 0)), (300001, (5, 12, 0)), (300001, (0, 0, 0))]:
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        got = dev.run(op, a, b, offs, dst_is=which)
        assert np.array_equal(got, _ref(op, a, b)), (op, n, offs, which)


def test_a_grid_of_two_workgroups_strides(monkeypatch):
    """300,001 bytes are 19 tiles: with VF_MAX_BLOCKS = 2 every workgroup takes 9 or 10 of them."""
    monkeypatch.setenv("VF_MAX_BLOCKS", "2")
    rng = np.random.default_rng(23)
    n = 300001
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    with vfilter.Context(0, max_frame_bytes=1 << 20, max_batch=1) as ctx:
        d = _Dev(ctx, n)
        try:
            for op in OPS:
                for offs in ALIGNMENTS[:2]:
                    assert np.array_equal(d.run(op, a, b, offs), _ref(op, a, b)), (op, offs)
            assert np.array_equal(d.run("subtract", a, b, (7, 7, 0), dst_is="a"), _ref("subtract", a, b))
        finally:
            d.close()


def test_refusals_and_the_empty_range(dev, vf_ctx):
    lib = _lib.load_library()
    h = vf_ctx.handle
    pa, pb, pd = (p + PAD for p in dev.bufs)
    n = 4096
    a = np.arange(n, dtype=np.uint32).astype(np.uint8)
    b = a[::-1].copy()

    def still_works():
        assert np.array_equal(dev.run("absdiff", a, b, (1, 5, 11)), _ref("absdiff", a, b))

    for args, word in [((pa, pb, pa + 1, n, 0), b"partially overlaps"), ((pa, pb, pb + n - 1, n, 1), b"partially overlaps"),
                       ((pa + 8, pb, pa, n, 2), b"partially overlaps"),
                       ((None, pb, pd, n, 0), b"NULL"), ((pa, None, pd, n, 0), b"NULL"), ((pa, pb, None, n, 0), b"NULL"),
                       ((pa, pb, pd, n, 5), b"unknown op 5"), ((pa, pb, pd, n, -1), b"unknown op -1"),
                       ((pa, pb, pd, 0, 9), b"unknown op 9")]:
        assert lib.vf_binary_device(h, *args, None) == _lib.VF_E_INVALID, args
        assert word in lib.vf_last_error(None), (args, lib.vf_last_error(None))
        assert word in lib.vf_last_error(h)
        still_works()
    assert lib.vf_binary_device(None, pa, pb, pd, n, 0, None) == _lib.VF_E_INVALID
    # nbytes == 0: VF_OK, nothing written, NULL pointers and all
    vf_ctx.memset_device(dev.bufs[2], 0xEE, dev.size)
    vf_ctx.sync()
    assert lib.vf_binary_device(h, pa, pb, pd, 0, 0, None) == _lib.VF_OK
    assert lib.vf_binary_device(h, None, None, None, 0, 4, None) == _lib.VF_OK
    vf_ctx.sync()
    got = np.empty(dev.size, np.uint8)
    vf_ctx.download(got, dev.bufs[2], dev.size)
    vf_ctx.sync()
    assert np.all(got == 0xEE)
    # an operand may be the other operand, and ranges that only touch do not overlap
    assert lib.vf_binary_device(h, pa, pa, pd, n, 4, None) == _lib.VF_OK
    assert lib.vf_binary_device(h, pa, pa + n, pa + 2 * n, n, 0, None) == _lib.VF_OK
    vf_ctx.sync()
    still_works()
