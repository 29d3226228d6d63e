"""The Python values of the level filter, without a GPU context: ``Level``'s validation and its messages,
its lowering to step tuples, ``Chain`` / ``Combine`` with a ``Level``, ``LevelWorker``'s options -- and
``tests/_level_ref.py`` itself on cases worked out by hand, since every GPU test leans on it.
"""
import numpy as np
import pytest

import _level_ref as R
from vfilter import Level, filters
from vfilter.filters import STEP_BINARY, STEP_LEVEL, STEP_TABLE, Chain, Combine, Invert, Kernel
from vfilter.level_worker import LevelWorker, level_from_options, main


def test_level_values():
    e = Level.equalize()
    assert e.family == "level" and e.args == (0, 0, 0, 0, 0) and e.rule == "equalize" and e.min_channels == 1
    s = Level.stretch(0.01, channels=(0, 2), link=True)
    assert s.args == (1, 5, 1, 655, 655) and s.rule == "stretch" and s.link is True and s.min_channels == 3
    assert Level.stretch((0.25, 0.0)).args == (1, 0, 0, 16384, 0)
    assert Level.stretch(32767 / 65536).args == (1, 0, 0, 32767, 32767)
    assert Level.stretch(0.49999).clip_lo == 32767  # int(round(f * 65536)), at the limit
    assert Level.equalize(channels=1).mask == 2 and Level.equalize(channels=[2, 0]).mask == 5
    assert Level.equalize(channels=(0,)).min_channels == 1
    assert Level("stretch", clip=0.0).args == (1, 0, 0, 0, 0)
    with pytest.raises(dataclasses_error()):
        e.mask = 3
    assert filters.STEP_LEVEL == 8 and filters.LEVEL_RULES == {"equalize": 0, "stretch": 1}


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


@pytest.mark.parametrize("kwargs,word", [
    (dict(rule="gamma"), "rule must be one of"),
    (dict(rule="stretch", clip=0.5), "a clip is a fraction in [0, 0.5)"),
    (dict(rule="stretch", clip=-0.1), "a clip is a fraction in [0, 0.5)"),
    (dict(rule="stretch", clip=float("nan")), "a clip is a fraction in [0, 0.5)"),
    (dict(rule="stretch", clip=0.499999), "at most 32767 / 65536"),
    (dict(rule="stretch", clip=(0.1, 0.2, 0.3)), "clip is a fraction or (lo, hi)"),
    (dict(rule="stretch", clip="much"), "clip is a fraction or (lo, hi)"),
    (dict(rule="equalize", clip=0.01), "the equalize rule takes no clip"),
    (dict(rule="equalize", channels=()), "distinct indices among 0, 1, 2"),
    (dict(rule="equalize", channels=(3,)), "distinct indices among 0, 1, 2"),
    (dict(rule="equalize", channels=(0, 0)), "distinct indices among 0, 1, 2"),
    (dict(rule="equalize", channels=(-1,)), "distinct indices among 0, 1, 2"),
    (dict(rule="equalize", channels=(0.5,)), "channels is None or channel indices"),
    (dict(rule="equalize", channels=(True,)), "channels is None or channel indices"),
    (dict(rule="equalize", link=1), "link is a bool"),
])
def test_level_refuses(kwargs, word):
    with pytest.raises(ValueError) as e:
        Level(**kwargs)
    assert word in str(e.value), str(e.value)


def test_lowering_to_steps():
    c = Chain([Level.stretch(0.01, (1,), True)])
    assert c.steps == ((STEP_LEVEL, 0, 0, 1, (2, 1, 655, 655), 0, 0),) and c.level_channels == 3 and c.family == "chain"
    c = Chain([Invert(), Level.equalize(), Kernel(np.ones((3, 3)))])
    assert [st[0] for st in c.steps] == [STEP_TABLE, STEP_LEVEL, 1] and [st[1] for st in c.steps] == [0, 1, 2]
    assert c.steps[1][3:5] == (0, (0, 0, 0, 0)) and c.level_channels == 1
    c = Chain(Combine("max", None, Level.equalize(link=True)))
    assert c.steps == ((STEP_LEVEL, 0, 0, 0, (0, 1, 0, 0), 0, 0), (STEP_BINARY, 0, 1, 4, None, 0, 0))
    c = Chain(Combine("absdiff", Level.equalize(), Chain([Level.stretch(0.1), Invert()])))
    assert [st[0] for st in c.steps] == [STEP_LEVEL, STEP_LEVEL, STEP_TABLE, STEP_BINARY] and c.steps[3][1:3] == (1, 3)
    c = Chain.program([(Level.equalize(), 0), (Level.stretch(), 0), ("add", 1, 2)])
    assert c.steps[1] == (STEP_LEVEL, 0, 0, 1, (0, 0, 0, 0), 0, 0)
    with pytest.raises(ValueError, match="a step is Invert, Table, Kernel, Rank, Mix, Separable, Level, Combine or Chain"):
        Chain(["equalize"])
    with pytest.raises(ValueError):
        Combine("max", "equalize")
    with pytest.raises(ValueError, match="channel 1 or 2"):
        filters._chain_frame("chain", np.zeros((4, 4), np.uint8), Chain(Level.equalize((2,))))
    with pytest.raises(ValueError, match="level is a Level"):
        filters.level_frames([], "equalize")


def test_worker_options():
    assert level_from_options(equalize=True).args == (0, 0, 0, 0, 0)
    assert level_from_options(stretch=[0.01], channels=[0, 1], link=True).args == (1, 3, 1, 655, 655)
    assert level_from_options(stretch=[0.0, 0.25]).args == (1, 0, 0, 0, 16384)
    for bad in (dict(), dict(equalize=True, stretch=[0.1]), dict(stretch=[0.1, 0.2, 0.3]), dict(stretch=[0.5]),
                dict(equalize=True, channels=[3]), dict(equalize=True, channels=[1, 1])):
        with pytest.raises(ValueError):
            level_from_options(**bad)
    with pytest.raises(ValueError, match="level is a vfilter.filters.Level"):
        LevelWorker("127.0.0.1", 1, 1, 0.0, level="equalize", install_signal_handlers=False, transport="tcp")
    for argv in (["--equalize", "--stretch", "0.1"], [], ["--stretch", "0.7"], ["--equalize", "--channels", "5"]):
        with pytest.raises((ValueError, SystemExit)):  # a bad combination ends before a GPU context exists
            main(["127.0.0.1", "5555", "5556"] + argv)


def test_the_reference_by_hand():
    img = np.array([[52, 55, 61, 59], [79, 61, 76, 61], [55, 52, 52, 52]], np.uint8)
    h = R.hist(img)
    assert h.shape == (1, 256) and h[0, 52] == 4 and h[0, 61] == 3 and h.sum() == 12
    # cv2.equalizeHist by hand: i0 = 52, scale = 255 / 8, the sums above 52 are 2, 3, 6, 7, 8
    want = {52: 0, 55: 64, 59: 96, 61: 191, 76: 223, 79: 255}
    out = R.level(img, R.EQUALIZE)
    assert all(out[img == v].tolist() == [w] * int((img == v).sum()) for v, w in want.items())
    # min-max: lo = 52, hi = 79, (510 (v - 52) + 27) // 54
    st = R.level(img, R.STRETCH)
    assert st[0].tolist() == [0, 28, 85, 66] and st.max() == 255
    # a clip of a quarter at the dark end: cut_lo = 3, so lo = 52 still (4 entries > 3); a third: lo = 55
    assert np.array_equal(R.level(img, R.STRETCH, 0, 0, (16384, 0)), st)
    assert R.level(img, R.STRETCH, 0, 0, (21846, 0))[0, 1] == 0
    rgb = np.stack([img, img // 2, 255 - img], axis=2)
    one = R.level(rgb, R.EQUALIZE, 2)
    assert np.array_equal(one[:, :, 0], rgb[:, :, 0]) and np.array_equal(one[:, :, 2], rgb[:, :, 2])
    assert np.array_equal(one[:, :, 1], R.level(rgb[:, :, 1].copy(), R.EQUALIZE))
    linked = R.level(rgb, R.STRETCH, 5, 1)
    t = R.table(R.hist(rgb)[0].astype(np.int64) + R.hist(rgb)[2], 24, R.STRETCH)
    assert np.array_equal(linked[:, :, 0], t[rgb[:, :, 0]]) and np.array_equal(linked[:, :, 1], rgb[:, :, 1])
    assert R.level(np.empty((0, 0, 3), np.uint8), R.EQUALIZE).shape == (0, 0, 3)
