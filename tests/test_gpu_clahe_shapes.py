"""CLAHE at the geometry a production frame has: tile rows wider than a workgroup, histogram slices taller than
``kRows``, and cells that the blend cuts unevenly.  Every frame of ``tests/test_gpu_clahe*.py`` has at most 180
bytes a tile row and at most four rows a slice, so there the two column loops of ``csrc/vf_clahe.hip`` run one
pass and the histogram's row loop one round; 1920 x 1080 under 8 x 8 has 720 bytes (three passes, and a lane's
channel changes from pass to pass because 256 % 3 = 1) and 9 rows (rounds of 4, 4 and 1).  The frames here are the
smallest that reach each of those loops (``tests/_clahe_shapes.py``); ``test_the_frames_are_what_they_are_chosen_for``
needs no GPU and holds the arithmetic, so a later retune of a constant fails it with a reason instead of leaving
the GPU tests passing without a second pass.

Everything runs at the default switches, on the session's context, against ``tests/_clahe_ref.py``; every
comparison is exact.  Contents are ``test_gpu_clahe.py``'s: ``random``; ``tile_constants``, every tile its own
table, where a slipped column or tile index shows; ``channel_constants``, where a channel slip on a later pass
changes every byte; ``two_values``, where the clip bites.
"""
import numpy as np
import pytest

import _clahe_shapes as S
from _clahe_shapes import CASES
from test_gpu_clahe import _filter, _frame, _want

gpu = pytest.mark.gpu

CONTENTS = ["random", "tile_constants", "channel_constants", "two_values"]
LIMITS = [0, 512, 10240]
WIDE = ["a", "c"]  # the cases with a second pass of columns: these also run on device buffers, in place and masked


def test_the_frames_are_what_they_are_chosen_for():
    assert S.constants_in_the_sources() == (S.K_BLOCK, S.K_ROWS, S.HIST_TARGET, S.APPLY_TARGET, S.REPLICAS) == \
        (256, 4, 1024, 512, 8)
    p = {(k, c): S.plan(h, w, grid, c) for k, (h, w, grid) in CASES.items() for c in (1, 3)}
    # the table of the cases: a tile, the histogram's slices, the blend's strips
    assert [(p[k, 1].th, p[k, 1].tw, p[k, 1].slices, p[k, 1].rows, p[k, 1].last_slice, p[k, 1].strips) for k in "abcd"] == \
        [(20, 260, 20, 1, 1, 20), (21, 4, 4, 6, 3, 2), (37, 90, 8, 5, 2, 4), (35, 3, 4, 9, 8, 2)]
    # the histogram's column loop: a second pass on one channel and on three; a last pass narrower than 16 lanes
    assert S.passes(p["a", 1].hist_bytes) == (2, 4) and S.passes(p["a", 3].hist_bytes) == (4, 12)
    assert S.passes(p["c", 1].hist_bytes) == (1, 90) and S.passes(p["c", 3].hist_bytes) == (2, 14)
    for c in (1, 3):
        assert any(p[k, c].hist_bytes > S.K_BLOCK for k in CASES), c
    # the blend's column loop, over a cell's columns: case a has cells of 130, 260 and 130 columns, so on three
    # channels 390 bytes, whose last pass of 134 lanes is wider than a wave, and 780, whose last has 12
    assert p["a", 1].cell_w == [130, 260, 130] and p["a", 1].cell_h == [10, 20, 10]
    assert [S.passes(wd * 3) for wd in p["a", 3].cell_w] == [(2, 134), (4, 12), (2, 134)]
    assert [S.passes(wd) for wd in p["a", 1].cell_w] == [(1, 130), (2, 4), (1, 130)]
    assert max(p["c", 3].cell_w) == 90 and S.passes(90 * 3) == (2, 14) and S.passes(90) == (1, 90)
    last = [S.passes(wd * c)[1] for (k, c), q in p.items() for wd in q.cell_w if S.passes(wd * c)[0] > 1]
    assert min(last) < 16 and max(last) > 64
    # the histogram's row loop: rounds of kRows rows, the last one partial
    assert S.rounds(p["b", 1].rows) == [4, 2] and S.rounds(p["b", 1].last_slice) == [3]
    assert S.rounds(p["c", 1].rows) == [4, 1] and S.rounds(p["c", 1].last_slice) == [2]
    assert S.rounds(p["d", 1].rows) == [4, 4, 1] and S.rounds(p["d", 1].last_slice) == [4, 4]
    assert S.rounds(S.plan(1080, 1920, (8, 8), 3).rows) == [4, 4, 1]  # what case d stands for
    assert S.passes(S.plan(1080, 1920, (8, 8), 3).hist_bytes) == (3, 208)
    rows = {q.rows for q in p.values()}
    assert rows & {5, 6, 7} and max(rows) >= 9
    assert any(q.last_slice % S.K_ROWS and q.last_slice != q.rows for q in p.values())
    for q in p.values():  # the slices cover the tile, and none is empty
        assert (q.slices - 1) * q.rows < q.th <= q.slices * q.rows and 1 <= q.last_slice <= q.rows
    # the blend's strips: case a has 20 strips over cells of 10 rows, so 10 of them return early; case b cuts cells
    # of 21 rows into 11 and 10
    assert S.strip_cut(10, p["a", 1].strips) == ([1] * 10, 10) and S.strip_cut(20, p["a", 1].strips) == ([1] * 20, 0)
    assert sorted(set(p["b", 1].cell_h)) == [4, 11, 21] and p["b", 1].strips == 2  # the frame ends 4 rows past a centre
    assert S.strip_cut(21, 2) == ([11, 10], 0) and S.strip_cut(11, 2) == ([6, 5], 0) and S.strip_cut(4, 2) == ([2, 2], 0)
    assert any(len(set(S.strip_cut(hh, q.strips)[0])) > 1 for q in p.values() for hh in q.cell_h)
    assert any(S.strip_cut(hh, q.strips)[1] > 0 for q in p.values() for hh in q.cell_h)
    # case c divides on neither axis, and the reflected margin of its last tile column, bytes 255 .. 269 of the tile
    # row on three channels, ends in the second pass
    h, w, grid = CASES["c"]
    assert h % grid[1] and w % grid[0] and (w - 7 * 90) * 3 == 255 and 90 * 3 > S.K_BLOCK
    # the contents do what they are there for: nearly every tile its own table, and the clip changes the picture
    img = _frame("tile_constants", h, w, 1, grid)
    tabs = S.R.tile_tables(img, 512, *grid)
    assert len({tabs[ty, tx].tobytes() for ty in range(grid[1]) for tx in range(grid[0])}) >= 100
    two = _frame("two_values", 40, 520, 1, (2, 2))
    assert not np.array_equal(_want(("two_values", 40, 520, 1), two, 10240, (2, 2)), _want(("two_values", 40, 520, 1), two, 0, (2, 2)))


@gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_content_and_limit(vf_ctx, case, c):
    import vfilter
    h, w, grid = CASES[case]
    for content in CONTENTS:
        img = _frame(content, h, w, c, grid)
        for q in LIMITS:
            out = vfilter.clahe_frames([img], _filter(q, grid), ctx=vf_ctx)[0]
            want = _want((content, h, w, c), img, q, grid)
            assert out.shape == img.shape and np.array_equal(out, want), (case, content, q, np.argwhere(out != want)[:5])


@gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("so,do", [(0, 0), (7, 7), (3, 8)])
@pytest.mark.parametrize("case", WIDE)
def test_device_buffers_off_the_16_byte_grid(vf_ctx, case, so, do, c):
    """Canaries on both sides: a later pass may not write past a row's or the frame's last byte."""
    h, w, grid = CASES[case]
    img = _frame("random", h, w, c, grid)
    n = img.nbytes
    got = np.empty(n + 64, np.uint8)
    dsrc, ddst = vf_ctx.alloc_device(n + 64), vf_ctx.alloc_device(n + 64)
    try:
        vf_ctx.memset_device(ddst, 0xEE, n + 64)
        vf_ctx.upload(dsrc + so, img, n)
        vf_ctx.clahe_device(dsrc + so, ddst + 16 + do, w, h, c, 512, grid[0], grid[1], 0)
        vf_ctx.sync()
        vf_ctx.download(got, ddst, n + 64)
        vf_ctx.sync()
    finally:
        for p in (dsrc, ddst):
            vf_ctx.free_device(p)
    lo = 16 + do
    assert np.array_equal(got[lo:lo + n].reshape(img.shape), _want(("random", h, w, c), img, 512, grid))
    assert np.all(got[:lo] == 0xEE) and np.all(got[lo + n:] == 0xEE)


@gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("case", WIDE)
def test_in_place(vf_ctx, case, c):
    import vfilter
    h, w, grid = CASES[case]
    img = _frame("tile_constants", h, w, c, grid)
    want = _want(("tile_constants", h, w, c), img, 512, grid)
    buf = img.copy()
    assert vfilter.clahe(buf, 2.0, grid, dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, want)
    n = img.nbytes
    got = np.empty_like(img)
    d = vf_ctx.alloc_device(n)
    try:
        vf_ctx.upload(d, img, n)
        vf_ctx.clahe_device(d, d, w, h, c, 512, grid[0], grid[1], 0)  # dst is src on the device
        vf_ctx.sync()
        vf_ctx.download(got, d, n)
        vf_ctx.sync()
    finally:
        vf_ctx.free_device(d)
    assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("mask", [2, 5])
@pytest.mark.parametrize("case", WIDE)
def test_masks(vf_ctx, case, mask):
    """A channel outside the mask takes the histogram's ``continue`` on every pass and is copied by the blend's
    column loop: it comes back unchanged, and the others as if they were alone."""
    import vfilter
    h, w, grid = CASES[case]
    for content in ("random", "channel_constants"):
        img = _frame(content, h, w, 3, grid)
        got = vfilter.clahe_frames([img], _filter(512, grid, mask), ctx=vf_ctx)[0]
        want = _want((content, h, w, 3), img, 512, grid, mask)
        assert np.array_equal(got, want), (case, content, mask, np.argwhere(got != want)[:5])
        for ch in range(3):
            if not mask >> ch & 1:
                assert np.array_equal(got[:, :, ch], img[:, :, ch]), (case, content, mask, ch)
            else:
                assert np.array_equal(got[:, :, ch], _want((content, h, w, 3), img, 512, grid)[:, :, ch])


@gpu
@pytest.mark.parametrize("c", [1, 3])
def test_case_a_as_a_step_of_a_chain(vf_ctx, c):
    import vfilter
    from vfilter.filters import Invert
    h, w, grid = CASES["a"]
    img = _frame("tile_constants", h, w, c, grid)
    want = 255 - _want(("tile_constants", h, w, c), img, 512, grid)
    got = vfilter.chain(img, [_filter(512, grid), Invert()], ctx=vf_ctx)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    buf = img.copy()
    assert vfilter.chain(buf, [_filter(512, grid), Invert()], dst=buf, ctx=vf_ctx) is buf and np.array_equal(buf, want)


@gpu
def test_case_a_through_the_jpeg_path(vf_ctx):
    """Decode, CLAHE and encode on the GPU against the oracle composition of ``tests/test_gpu_clahe_jpeg.py``: whole
    JPEG byte strings are compared."""
    from oracle import jpeg as J
    from vfilter.jpeg import TurboJPEG
    h, w, grid = CASES["a"]
    tj = TurboJPEG(ctx=vf_ctx)
    j = J.encode(J.synthetic_scene(97, h, w), 90, J.TJPF_BGR, J.TJSAMP_422)
    bgr = J.decode(j, J.TJPF_BGR, 0)
    assert bgr.shape == (h, w, 3)
    for q in (512, 10240):
        want = J.encode(S.R.clahe(bgr, q, grid[0], grid[1], 0), 85, J.TJPF_BGR, J.TJSAMP_422, 0, 3)
        assert tj.filter_batch([j], _filter(q, grid))[0] == want, q
