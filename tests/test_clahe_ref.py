"""The Python values of CLAHE, without a GPU context: ``Clahe``'s validation and its messages, its lowering to
step tuples, ``Chain`` / ``Combine`` with a ``Clahe``, ``create_clahe``'s getters, ``ClaheWorker``'s options -- and
``tests/_clahe_ref.py`` itself on cases worked out by hand, since every GPU test leans on it.
"""
import dataclasses

import numpy as np
import pytest

import _clahe_ref as R
import vfilter
from vfilter import Clahe, filters
from vfilter.clahe_worker import ClaheWorker, main
from vfilter.filters import STEP_BINARY, STEP_CLAHE, STEP_TABLE, Chain, Combine, Invert, Kernel, Level


def test_clahe_values():
    d = Clahe()
    assert d.family == "clahe" and d.args == (10240, 8, 8, 0) and d.clip_limit == 40.0 and d.min_channels == 1  # cv2's defaults
    assert Clahe(2.0).args == (512, 8, 8, 0) and Clahe(2.5).args == (640, 8, 8, 0) and Clahe(4.0).clip_q8 == 1024
    assert Clahe(0).args == (0, 8, 8, 0) and Clahe(1 / 256).clip_q8 == 1 and Clahe(65536).clip_q8 == 1 << 24
    f = Clahe(2.0, (16, 3), channels=(0, 2))
    assert f.args == (512, 16, 3, 5) and (f.tiles_x, f.tiles_y) == (16, 3) and f.min_channels == 3
    assert Clahe(2.0, channels=1).mask == 2 and Clahe(2.0, channels=[0]).min_channels == 1
    assert Clahe(np.float32(2.5), np.array([4, 2])).args == (640, 4, 2, 0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.mask = 3
    assert filters.STEP_CLAHE == 10 and vfilter._lib.STEP_CLAHE == 10


@pytest.mark.parametrize("kwargs,word", [
    (dict(clip_limit=0.3), "clip_limit * 256 must be an integer"),
    (dict(clip_limit=2.001), "clip_limit * 256 must be an integer"),
    (dict(clip_limit=-1), "a clip limit is in [0, 65536]"),
    (dict(clip_limit=-1 / 256), "a clip limit is in [0, 65536]"),
    (dict(clip_limit=65536.5), "a clip limit is in [0, 65536]"),
    (dict(clip_limit=float("nan")), "a clip limit is in [0, 65536]"),
    (dict(clip_limit="high"), "clip_limit is a number"),
    (dict(clip_limit=True), "clip_limit is a number"),
    (dict(tile_grid_size=(0, 8)), "1 .. 16 tiles an axis"),
    (dict(tile_grid_size=(8, 17)), "1 .. 16 tiles an axis"),
    (dict(tile_grid_size=(17, 8)), "1 .. 16 tiles an axis"),
    (dict(tile_grid_size=(-8, 8)), "1 .. 16 tiles an axis"),
    (dict(tile_grid_size=8), "tile_grid_size is (tiles_x, tiles_y)"),
    (dict(tile_grid_size=(8, 8, 8)), "tile_grid_size is (tiles_x, tiles_y)"),
    (dict(tile_grid_size=(8.5, 8)), "tile_grid_size is (tiles_x, tiles_y)"),
    (dict(tile_grid_size=(True, 8)), "tile_grid_size is (tiles_x, tiles_y)"),
    (dict(channels=(3,)), "distinct indices among 0, 1, 2"),
    (dict(channels=3), "distinct indices among 0, 1, 2"),
    (dict(channels=()), "distinct indices among 0, 1, 2"),
    (dict(channels=(1, 1)), "distinct indices among 0, 1, 2"),
    (dict(channels=(True,)), "channels is None or channel indices"),
    (dict(channels=True), "channels is None or channel indices"),
])
def test_clahe_refuses(kwargs, word):
    with pytest.raises(ValueError) as e:
        Clahe(**kwargs)
    assert word in str(e.value) and str(e.value).startswith("Clahe:"), str(e.value)


def test_create_clahe_is_the_cv2_object():
    obj = vfilter.create_clahe(2.0, (8, 8))
    assert obj.getClipLimit() == 2.0 and obj.getTilesGridSize() == (8, 8)
    assert vfilter.create_clahe().getClipLimit() == 40.0 and vfilter.create_clahe().getTilesGridSize() == (8, 8)
    obj.setClipLimit(2.5)
    obj.setTilesGridSize((4, 2))
    assert obj.getClipLimit() == 2.5 and obj.getTilesGridSize() == (4, 2)
    with pytest.raises(ValueError):
        vfilter.create_clahe(0.3)
    with pytest.raises(ValueError):
        obj.setTilesGridSize((0, 1))
    assert obj.apply(np.empty((0, 0), np.uint8)).shape == (0, 0)  # the empty frame needs no context


def test_lowering_to_steps():
    c = Chain([Clahe(2.0, (4, 2), (1,))])
    assert c.steps == ((STEP_CLAHE, 0, 0, 0, (2, 512, 4, 2), 0, 0),) and c.level_channels == 3 and c.family == "chain"
    c = Chain([Invert(), Clahe(), Kernel(np.ones((3, 3)))])
    assert [st[0] for st in c.steps] == [STEP_TABLE, STEP_CLAHE, 1] and [st[1] for st in c.steps] == [0, 1, 2]
    assert c.steps[1][3:5] == (0, (0, 10240, 8, 8)) and c.level_channels == 1
    c = Chain(Combine("max", None, Clahe(2.0)))
    assert c.steps == ((STEP_CLAHE, 0, 0, 0, (0, 512, 8, 8), 0, 0), (STEP_BINARY, 0, 1, 4, None, 0, 0))
    c = Chain(Combine("absdiff", Clahe(2.0), Chain([Level.equalize(), Clahe(4.0, (2, 2))])))
    assert [st[0] for st in c.steps] == [STEP_CLAHE, 8, STEP_CLAHE, STEP_BINARY] and c.steps[3][1:3] == (1, 3)
    with pytest.raises(ValueError, match="Level, Combine or Chain, or a Clahe, not str"):
        Chain(["clahe"])
    with pytest.raises(ValueError, match="channel 1 or 2"):
        filters._chain_frame("chain", np.zeros((4, 4), np.uint8), Chain(Clahe(2.0, channels=(2,))))
    with pytest.raises(ValueError, match="the filter is a Clahe"):
        filters.clahe_frames([], "clahe")
    with pytest.raises(ValueError, match="channel 1 or 2"):
        filters.clahe(np.zeros((4, 4), np.uint8), 2.0, channels=(1,))


def test_worker_options():
    with pytest.raises(ValueError, match="clahe is a vfilter.filters.Clahe"):
        ClaheWorker("127.0.0.1", 1, 1, 0.0, clahe="clahe", install_signal_handlers=False, transport="tcp")
    for argv in (["--clip-limit", "0.3"], ["--tiles", "0", "8"], ["--tiles", "8"], ["--channels", "5"],
                 ["--clip-limit", "-2"], ["--tiles", "8", "17"]):
        with pytest.raises((ValueError, SystemExit)):  # a bad value ends before a GPU context exists
            main(["127.0.0.1", "5555", "5556"] + argv)


def test_a_1_x_1_grid_is_the_table_itself():
    """One tile: both tile indices clamp to it on both axes, the four entries are the same e, and
    (e xa1 + e xa) ya1 + (e xa1 + e xa) ya must round back to e for every weight that occurs."""
    rng = np.random.default_rng(3)
    for h, w in [(97, 53), (1, 1), (7, 300), (64, 64)]:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for q in (0, 256, 512, 10240):
            tab = R.tile_tables(img, q, 1, 1)[0, 0]
            assert np.array_equal(R.clahe(img, q, 1, 1), tab[img]), (h, w, q)


def test_the_reference_by_hand():
    # one 2 x 4 tile, area 8: values 10 x 5, 20 x 2, 30 x 1
    img = np.array([[10, 10, 10, 20], [10, 10, 20, 30]], np.uint8)
    assert R.geometry(2, 4, 1, 1) == (2, 4, 2, 4)
    # no clipping: the sums are 5, 7, 8, scale = 255 / 8: rint(159.375), rint(223.125), 255
    t = R.tile_tables(img, 0, 1, 1)[0, 0]
    assert (t[9], t[10], t[19], t[20], t[29], t[30], t[255]) == (0, 159, 159, 223, 223, 255, 255)
    # a limit of 64: clip = max(64 * 256 * 8 >> 16, 1) = 2; the excess is 3, batch 0, residual 3, step 85: bins 0, 85
    # and 170 gain one.  The bins are then 1 at 0, 2 at 10, 2 at 20, 1 at 30, 1 at 85, 1 at 170
    assert R.clip_of(64 * 256, 8) == 2
    r = R.redistribute(np.bincount(img.ravel(), minlength=256), 2)
    assert sum(r) == 8 and (r[0], r[10], r[20], r[30], r[85], r[170]) == (1, 2, 2, 1, 1, 1)
    t = R.tile_tables(img, 64 * 256, 1, 1)[0, 0]
    assert (t[0], t[10], t[20], t[30], t[85], t[170]) == (32, 96, 159, 191, 223, 255)  # rint(31.875 k), halves to even none
    # geometry: the full-tile pad, and a margin that reflects without the edge pixel
    assert R.geometry(66, 64, 8, 8) == (72, 72, 9, 9) and R.geometry(3, 300, 16, 1) == (4, 304, 4, 19)
    assert [R.reflect101(p, 5) for p in range(5, 9)] == [3, 2, 1, 0] and R.reflect101(9, 5) == 1
    # the weights of a tile of 4 on an axis of 8 with 2 tiles: txf = x / 4 - 0.5
    t1, t2, a, a1 = R.weights(8, 4, 2)
    assert t1.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and t2.tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert a.tolist() == [0.5, 0.75, 0.0, 0.25, 0.5, 0.75, 0.0, 0.25] and a1.tolist() == [0.5, 0.25, 1.0, 0.75, 0.5, 0.25, 1.0, 0.75]
    assert a.dtype == np.float32 and a1.dtype == np.float32
    # the blend: a half rounds to even, and the sum of float32 products stays float32
    assert int(R.blend(1, 2, 1, 2, np.float32(0.5), np.float32(0.5), np.float32(0.0), np.float32(1.0))) == 2  # 1.5
    assert int(R.blend(2, 3, 2, 3, np.float32(0.5), np.float32(0.5), np.float32(0.0), np.float32(1.0))) == 2  # 2.5
    assert R.blend(np.array([7]), 7, 7, 7, np.float32(0.3), np.float32(0.7), np.float32(0.1), np.float32(0.9)).dtype == np.uint8
    # masks, channels and the empty frame
    rgb = np.stack([img, img * 2, 255 - img], axis=2)
    one = R.clahe(rgb, 512, 2, 1, 2)
    assert np.array_equal(one[:, :, 0], rgb[:, :, 0]) and np.array_equal(one[:, :, 2], rgb[:, :, 2])
    assert np.array_equal(one[:, :, 1], R.clahe(rgb[:, :, 1].copy(), 512, 2, 1))
    assert R.clahe(np.empty((0, 0, 3), np.uint8), 512).shape == (0, 0, 3)
