"""The colour matrix on the CPU: the numpy reference of ``tests/_mix_ref.py`` against a float64
emulation, the ``vfilter.colors`` presets, ``as_matrix`` / ``Mix`` acceptance and refusals, and the
lowering of ``Mix`` into chain programs.  Nothing here needs a GPU or creates a context.
"""
import numpy as np
import pytest

import _mix_ref as M
from vfilter import Mix, as_matrix, colors, filters
from vfilter.filters import STEP_BINARY, STEP_MIX, STEP_RANK, STEP_TABLE, Chain, Combine, Invert, Rank, Table
from vfilter.mix_worker import mix_from_options

ROUNDINGS = ("half_even", "half_up")


def _plain(v):
    """A ``colors`` result as (int64 3 x 4, shift, the rounding it carries or None)."""
    if isinstance(v, Mix):
        return v.matrix.astype(np.int64), v.shift, v.rounding
    m, s = v
    return np.asarray(m, np.int64), s, None


def presets():
    return {"identity": colors.identity(), "swap_rb": colors.swap_rb(), "gray": colors.gray(),
            "gray_weights14": colors.gray_weights(1868, 9617, 4899, 14), "sepia": colors.sepia(),
            "saturation_half": colors.saturation(0.5), "saturation_0": colors.saturation(0),
            "saturation_1.75": colors.saturation(1.75), "gain": colors.gain(1, 1.5, 0.75),
            "offset": colors.offset(-20, 0, 255)}


def all_matrices():
    out = dict(M.matrix_set())
    for name, v in presets().items():
        m, s, _ = _plain(v)
        out["colors." + name] = (m, s)
    return out


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(2005)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8).reshape(2, 4, 3)
    return [rng.integers(0, 256, (37, 29, 3), dtype=np.uint8), corners, M.tie_frame()]


@pytest.mark.parametrize("name", sorted(all_matrices()))
def test_the_reference_equals_the_float64_emulation(frames, name):
    m, shift = all_matrices()[name]
    assert np.abs(m[:, :3]).sum(axis=1).max() <= 65536 and np.abs(m[:, 3]).max() <= 255 << shift
    for img in frames:
        for rounding in ROUNDINGS:
            got = M.mix(img, m, shift, rounding)
            assert got.dtype == np.uint8 and got.shape == img.shape
            assert np.array_equal(got, M.mix_float(img, m, shift, rounding)), (name, rounding)


def test_the_tie_matrix_has_ties_of_both_parities_and_the_roundings_differ_there():
    m, shift = M.TIES
    img = M.tie_frame()
    a = M.acc(img, m)
    f, r = a >> shift, a & ((1 << shift) - 1)
    tie = r == 1 << (shift - 1)
    even, odd = tie & (f % 2 == 0), tie & (f % 2 == 1)
    inside = (f >= 0) & (f < 255)  # the clamp hides nothing
    assert (even & inside).any() and (odd & inside).any()
    he, hu = M.descale(a, shift, "half_even"), M.descale(a, shift, "half_up")
    assert np.array_equal(he[even], f[even]) and np.array_equal(hu[even], f[even] + 1)  # they differ on even floors
    assert np.array_equal(he[odd], f[odd] + 1) and np.array_equal(hu[odd], f[odd] + 1)
    assert np.array_equal(he[~tie], hu[~tie])
    assert not np.array_equal(M.mix(img, m, shift, "half_even"), M.mix(img, m, shift, "half_up"))


def test_identity_swap_and_gray(frames):
    for img in frames:
        for rounding in ROUNDINGS:
            assert np.array_equal(M.mix(img, *M.IDENTITY, rounding), img)
            assert np.array_equal(M.mix(img, *M.SWAP_RB, rounding), img[..., ::-1])
        m, s, _ = _plain(colors.identity())
        assert np.array_equal(M.mix(img, m, s), img)
        m, s, _ = _plain(colors.swap_rb())
        assert np.array_equal(M.mix(img, m, s), img[..., ::-1])
        m, s, rounding = _plain(colors.gray())
        g = M.mix(img, m, s, rounding)
        assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
        x = img.astype(np.int64)
        assert np.array_equal(g[..., 0], (3735 * x[..., 0] + 19235 * x[..., 1] + 9798 * x[..., 2] + 16384) >> 15)


def test_the_presets_hold_the_integers_their_docstrings_give():
    g = colors.gray()
    assert g.rounding == "half_up" and g.shift == 15 and g.matrix.tolist() == [[3735, 19235, 9798, 0]] * 3
    m, s, r = _plain(colors.sepia())
    assert (s, r) == (8, None) and m.tolist() == [[34, 137, 70, 0], [43, 176, 89, 0], [48, 197, 101, 0]]
    m, s, _ = _plain(colors.saturation(0.5))
    assert s == 9 and m.tolist() == [[285, 150, 77, 0], [29, 406, 77, 0], [29, 150, 333, 0]]
    m, s, _ = _plain(colors.saturation(1))
    assert np.array_equal(M.mix(M.tie_frame(), m, s), M.tie_frame())
    m, s, _ = _plain(colors.gain(1, 1.5, 0.75))
    assert s == 2 and m.tolist() == [[4, 0, 0, 0], [0, 6, 0, 0], [0, 0, 3, 0]]
    m, s, _ = _plain(colors.offset(-20, 0, 255))
    assert s == 0 and m[:, 3].tolist() == [-20, 0, 255] and np.array_equal(m[:, :3], np.eye(3))
    m, s, _ = _plain(colors.gray_weights(1868, 9617, 4899, 14))
    assert s == 14 and m.tolist() == [[1868, 9617, 4899, 0]] * 3
    for bad in (lambda: colors.saturation(1 / 3), lambda: colors.saturation(-1), lambda: colors.gain(1, 2, 0.1),
                lambda: colors.offset(0, 0, 256), lambda: colors.offset(0.5, 0, 0),
                lambda: colors.gray_weights(1.0, 2, 3, 4)):
        with pytest.raises(ValueError):
            bad()
    for v in presets().values():  # every preset is Mix-ready
        mix = v if isinstance(v, Mix) else Mix(v)
        assert mix.matrix.dtype == np.int32 and mix.matrix.shape == (3, 4) and not mix.matrix.flags.writeable


def test_as_matrix_accepts():
    m, s = as_matrix(np.eye(3, dtype=np.int64))
    assert s == 0 and m.dtype == np.int32 and m.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    m, s = as_matrix(np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, -12]], np.int16))
    assert s == 0 and m[2].tolist() == [9, 10, 11, -12]
    m, s = as_matrix((np.array([[1, 2, 6, 2], [6, 2, 1, 2], [1, -2, 1, 2]]), 2))
    assert s == 2 and m[0].tolist() == [1, 2, 6, 2]
    m, s = as_matrix((np.full((3, 3), 4), 3))  # the smallest shift: 4 / 8 == 1 / 2
    assert s == 1 and m[0].tolist() == [1, 1, 1, 0]
    m, s = as_matrix(np.array([[0.5, 0.25, 0, 1.5], [0, 1, 0, 0], [0, 0, 1, 0]]))  # dyadic floats, offsets in pixels
    assert s == 2 and m[0].tolist() == [2, 1, 0, 6] and m[1].tolist() == [0, 4, 0, 0]
    m, s = as_matrix(np.eye(3))  # integral floats
    assert s == 0 and m[:, :3].tolist() == np.eye(3, dtype=int).tolist()
    m, s = as_matrix(np.full((3, 3), 2.0 ** -16))
    assert s == 16 and m[0].tolist() == [1, 1, 1, 0]
    m, s = as_matrix((M.matrix_set()["sum_65536_shift_16"][0], 16))
    assert s == 16 and int(np.abs(m[:, :3].astype(np.int64)).sum(axis=1).max()) == 65536


@pytest.mark.parametrize("bad, word", [
    (np.eye(4), "3 x 3 or 3 x 4"),
    (np.zeros((3,)), "3 x 3 or 3 x 4"),
    (np.zeros((2, 3)), "3 x 3 or 3 x 4"),
    ((np.eye(3), 1.5), "shift must be an integer"),
    ((np.eye(3), 17), "outside 0..16"),
    ((np.eye(3), -1), "outside 0..16"),
    ((np.eye(3) * 0.5, 2), "must be integers"),
    (np.full((3, 3), 1 / 3), "not dyadic"),
    (np.array([[0.299, 0.587, 0.114]] * 3), "not dyadic"),
    (np.full((3, 3), 2.0 ** -17), "not dyadic"),
    (np.array([[np.nan, 0, 0]] * 3), "non-finite"),
    (np.array([["a", "b", "c"]] * 3), "dtype"),
    (np.array([[32768, 0, 0], [0, 1, 0], [0, 0, 1]]), "does not fit 16 bits"),
    (np.array([[-32769, 0, 0], [0, 1, 0], [0, 0, 1]]), "does not fit 16 bits"),
    (np.array([[32767, 32767, 3], [0, 1, 0], [0, 0, 1]]), "exceeds 65536"),
    (np.array([[1, 0, 0, 256], [0, 1, 0, 0], [0, 0, 1, 0]]), "outside -255..255"),
    ((np.array([[1, 0, 0, -(255 * 4 + 1)], [0, 1, 0, 0], [0, 0, 1, 0]]), 2), "outside -255..255"),
])
def test_as_matrix_refuses_with_the_reason(bad, word):
    with pytest.raises(ValueError, match=word):
        as_matrix(bad)
    with pytest.raises(ValueError, match=word):
        Mix(bad)


def test_mix_is_a_frozen_copy_validated_when_constructed():
    src = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.int64)
    mix = Mix(src, "half_up")
    src[:] = 0  # copied
    assert mix.matrix[0].tolist() == [1, 2, 3, 4] and mix.family == "mix" and mix.rounding_code == 1
    assert Mix(np.eye(3)).rounding == "half_even" and Mix(np.eye(3)).rounding_code == 0
    assert mix.args[1:] == (0, 1) and mix.args[0] is mix.matrix
    with pytest.raises(ValueError):
        mix.matrix[0, 0] = 9  # read-only
    with pytest.raises(Exception):
        mix.shift = 3  # frozen
    with pytest.raises(ValueError, match="rounding must be one of"):
        Mix(np.eye(3), "nearest")
    with pytest.raises(ValueError, match="rounding must be one of"):
        Mix(np.eye(3), None)


def test_chain_lowering_of_mix():
    g, sep = colors.gray(), Mix(colors.sepia())
    c = Chain([g, Rank.median(3), sep])
    assert len(c) == 3 and c.has_mix and c.family == "chain"
    kind, a, b, op, data, shift, border = c.steps[0]
    assert (kind, a, b, op, shift, border) == (STEP_MIX, 0, 0, 1, 15, 0)
    assert data.dtype == np.int32 and data.shape == (3, 4) and np.array_equal(data, g.matrix)
    assert c.steps[1][0] == STEP_RANK and c.steps[2][:4] == (STEP_MIX, 2, 0, 0) and c.steps[2][5] == 8
    assert STEP_MIX == 5 and filters.STEP_MIX == 5  # 4 stays an unknown kind
    one = Chain(g)  # a bare filter value
    assert len(one) == 1 and one.steps[0][0] == STEP_MIX
    c = Chain([Combine("absdiff", g, None)])  # absdiff(gray x, x)
    assert [s[0] for s in c.steps] == [STEP_MIX, STEP_BINARY] and c.steps[1][1:3] == (1, 0) and c.has_mix
    c = Chain([Invert(), Combine("max", Chain([g, sep]), sep)])  # nested: a moved program keeps its operands
    assert [s[:3] for s in c.steps] == [(STEP_TABLE, 0, 0), (STEP_MIX, 1, 0), (STEP_MIX, 2, 0), (STEP_MIX, 1, 0),
                                        (STEP_BINARY, 3, 4)]
    c = Chain.program([(g, 0), (Rank.erode(), 1), ("subtract", 1, 2)])
    assert [s[0] for s in c.steps] == [STEP_MIX, STEP_RANK, STEP_BINARY] and c.has_mix
    assert not Chain([Invert(), Rank.median(3)]).has_mix and Chain([Table(np.arange(256, dtype=np.uint8))]).table_channels == 1
    with pytest.raises(ValueError, match="not a Mix|filter value"):
        Combine("add", colors.sepia(), None)  # a pair is not a filter value: Mix(...) makes one
    with pytest.raises(ValueError):
        Chain([colors.sepia()])


def test_one_channel_frames_are_refused_without_a_context():
    """Every refusal happens before a context is asked for: none exists on a machine without a GPU,
    and asking for one would raise ``VFilterError``, not ``ValueError``."""
    import vfilter
    g = colors.gray()
    for frame in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 1), np.uint8)):
        with pytest.raises(ValueError, match="H x W x 3"):
            vfilter.transform(frame, g)
        with pytest.raises(ValueError, match="H x W x 3"):
            vfilter.transform_frames([frame], g)
        with pytest.raises(ValueError, match="colour matrix"):
            vfilter.chain(frame, Chain([g, Rank.median(3)]))
        with pytest.raises(ValueError, match="colour matrix"):
            vfilter.chain_frames([frame], [Rank.median(3), g])
    with pytest.raises(ValueError):
        vfilter.transform(np.zeros((4, 5, 3), np.float32), g)
    with pytest.raises(ValueError, match="contradicts"):
        vfilter.transform(np.zeros((4, 5, 3), np.uint8), Mix(np.eye(3)), rounding="half_up")
    assert vfilter.transform(np.zeros((0, 5, 3), np.uint8), g).shape == (0, 5, 3)  # the empty frame: nothing to run


def test_the_worker_command_line_refuses_bad_combinations():
    assert mix_from_options("gray").rounding == "half_up"
    assert mix_from_options("sepia", (), "half_up").rounding == "half_up"
    assert mix_from_options("saturation", (0.5,)).shift == 9
    assert mix_from_options("offset", (1.0, -2.0, 3.0)).matrix[:, 3].tolist() == [1, -2, 3]
    for preset, params, rounding in (("gray", (), "half_even"), ("sepia", (1,), None), ("saturation", (), None),
                                     ("saturation", (1 / 3,), None), ("offset", (0.5, 0, 0), None), ("hue", (), None),
                                     ("gain", (1, 2), None), ("sepia", (), "nearest")):
        with pytest.raises(ValueError):
            mix_from_options(preset, params, rounding)
    from vfilter.mix_worker import MixWorker, _mix_shape
    with pytest.raises(ValueError, match="H W 3"):
        _mix_shape((480, 480))
    with pytest.raises(ValueError, match="Mix"):
        MixWorker("127.0.0.1", 1, 1, 0.0, use_jpeg=False, mix=colors.sepia(), install_signal_handlers=False,
                  transport="tcp")


def test_against_cv2_where_it_is_installed(frames):
    cv2 = pytest.importorskip("cv2")
    for img in frames:
        img = np.ascontiguousarray(img)
        m, s, r = _plain(colors.gray())
        assert np.array_equal(M.mix(img, m, s, r)[..., 0], cv2.cvtColor(img, cv2.COLOR_BGR2GRAY))
        for name in ("swap_rb", "shift0_offsets"):
            m, s = all_matrices()[name]
            assert np.array_equal(M.mix(img, m, s), cv2.transform(img, m.astype(np.float64) / (1 << s)))
