"""Filter chains on the CPU: the numpy interpreter of ``tests/_chain_ref.py`` against a plain triple
loop over the definition, so the reference the GPU tests compare with is itself
guarded; ``Morph`` against the documented step lists; what ``Chain``, ``Combine``, ``Morph`` and
``vfilter.chain`` refuse, all before any GPU work.  Where ``cv2`` is importable the reference's
``morph`` is also compared with ``cv2.morphologyEx`` (skipped otherwise)."""
import dataclasses

import numpy as np
import pytest

import _chain_ref as CR
import _rank_ref as R
import vfilter
from _chain_build import to_chain
from vfilter.filters import (BINARY_OPS, CHAIN_MAX_STEPS, STEP_BINARY, STEP_CONV, STEP_RANK, STEP_TABLE, Chain, Combine,
                             Invert, Kernel, Morph, Rank, Table)

NAMES = sorted(CR.program_set())


def _bidx(p, n, border):
    """The index tap position p reads on an axis of n, or None when the tap is outside (constant)."""
    if 0 <= p < n:
        return p
    if border == "constant":
        return None
    if border == "replicate":
        return 0 if p < 0 else n - 1
    if n == 1:
        return 0
    while p < 0 or p >= n:  # gfedcb|abcdefgh|gfedcba
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _round_half_even_shift(acc, shift):
    if shift == 0:
        return acc
    q, r = divmod(acc, 1 << shift)  # floor
    half = 1 << (shift - 1)
    return q + (1 if r > half or (r == half and q % 2 == 1) else 0)


def _loop_step(st, vals, shape):
    h, w, ch = shape
    out = np.empty(shape, np.uint8)
    for y in range(h):
        for x in range(w):
            for c in range(ch):
                if st[0] == "table":
                    t = np.asarray(st[2])
                    v = int(vals[st[1]][y, x, c])
                    out[y, x, c] = t[v] if t.ndim == 1 else t[v, c]
                elif st[0] == "bin":
                    a, b = int(vals[st[2]][y, x, c]), int(vals[st[3]][y, x, c])
                    r = {"subtract": a - b, "add": a + b, "absdiff": abs(a - b), "min": min(a, b), "max": max(a, b)}[st[1]]
                    out[y, x, c] = min(max(r, 0), 255)
                elif st[0] == "conv":
                    k = np.asarray(st[2])
                    kh, kw = k.shape
                    acc = 0
                    for j in range(kh):
                        for i in range(kw):
                            by, bx = _bidx(y + j - kh // 2, h, st[4]), _bidx(x + i - kw // 2, w, st[4])
                            if by is not None and bx is not None:  # constant: the tap reads 0
                                acc += int(k[j, i]) * int(vals[st[1]][by, bx, c])
                    out[y, x, c] = min(max(_round_half_even_shift(acc, st[3]), 0), 255)
                else:
                    op, arg, border = st[2], st[3], st[4]
                    e = np.ones((arg, arg), np.uint8) if op == "median" else np.asarray(arg)
                    border = "replicate" if op == "median" else border
                    kh, kw = e.shape
                    s = []
                    for j in range(kh):
                        for i in range(kw):
                            if e[j, i]:
                                by, bx = _bidx(y + j - kh // 2, h, border), _bidx(x + i - kw // 2, w, border)
                                if by is not None and bx is not None:  # constant: left out of the set
                                    s.append(int(vals[st[1]][by, bx, c]))
                    if op == "erode":
                        out[y, x, c] = min(s) if s else 255
                    elif op == "dilate":
                        out[y, x, c] = max(s) if s else 0
                    else:
                        out[y, x, c] = sorted(s)[len(s) // 2]
    return out


def _loop(img, prog):
    vals = [img]
    for st in prog:
        vals.append(_loop_step(st, vals, img.shape))
    return vals[-1]


@pytest.mark.parametrize("border", CR.BORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_the_interpreter_equals_a_triple_loop(name, border):
    for shape in [(7, 5, 3), (1, 1, 1)]:
        img = np.random.default_rng([len(name), shape[0]]).integers(0, 256, shape, dtype=np.uint8)
        prog = CR.program_set(border, shape[2])[name]
        assert np.array_equal(CR.run(img, prog), _loop(img, prog)), (name, border, shape)


def test_the_set_has_the_documented_shapes():
    ps = CR.program_set()
    assert len(ps) == 12
    assert len(ps["eight"]) == CR.MAX_STEPS == CHAIN_MAX_STEPS == 8
    assert len(ps["blackhat3_it2"]) == 5 and CR.reach(ps["blackhat3_it2"]) == 4
    assert CR.reach(ps["edges"]) == 2 and CR.reach(ps["diamond"]) == 3 and CR.reach(ps["pointwise"]) == 0
    # The inputs the GPU tests use are not degenerate: both zero and non-zero bytes come out.  Not so
    # for gradient_corner5 itself: a one-member element makes erode == dilate, and where the set is
    # empty max(0 - 255, 0) is 0 too, so that program is all zero on every input; corner5_reversed
    # subtracts the other way round and shows the edge.
    img = CR.noise(17, 13, 3)
    assert not CR.run(img, ps["gradient_corner5"]).any()
    rev = CR.run(img, ps["corner5_reversed"])
    assert (rev[:2] == 255).all() and (rev[:, :2] == 255).all() and not rev[2:, 2:].any()
    for out in (rev, CR.binary("subtract", img, CR.noise(17, 13, 3, seed=1))):
        assert (out == 0).any() and (out != 0).any()


def _shape(c):
    """(kind, a, b, op) per step: the structure of a Chain."""
    return [(k, a, b, op) for k, a, b, op, _d, _s, _b in c.steps]


def test_morph_flattens_to_the_documented_step_lists():
    E, D, SUB = 0, 1, BINARY_OPS["subtract"]
    rk = STEP_RANK
    assert _shape(Morph("erode", None, 3)) == [(rk, 0, 0, E), (rk, 1, 0, E), (rk, 2, 0, E)]
    assert _shape(Morph("dilate")) == [(rk, 0, 0, D)]
    assert _shape(Morph("open", None, 2)) == [(rk, 0, 0, E), (rk, 1, 0, E), (rk, 2, 0, D), (rk, 3, 0, D)]
    assert _shape(Morph("close")) == [(rk, 0, 0, D), (rk, 1, 0, E)]
    assert _shape(Morph("gradient", None, 2)) == [(rk, 0, 0, D), (rk, 1, 0, D), (rk, 0, 0, E), (rk, 3, 0, E),
                                                   (STEP_BINARY, 2, 4, SUB)]
    assert _shape(Morph("tophat")) == [(rk, 0, 0, E), (rk, 1, 0, D), (STEP_BINARY, 0, 2, SUB)]
    assert _shape(Morph("blackhat", None, 2)) == [(rk, 0, 0, D), (rk, 1, 0, D), (rk, 2, 0, E), (rk, 3, 0, E),
                                                   (STEP_BINARY, 4, 0, SUB)]
    # the element and the border reach every rank step; the default element is the 3 x 3 rectangle
    c = Morph("gradient", vfilter.elements.cross(5), 1, "replicate")
    for st in c.steps[:2]:
        assert np.array_equal(st[4], vfilter.elements.cross(5)) and st[6] == vfilter.filters.BORDERS["replicate"]
    assert np.array_equal(Morph("open").steps[0][4], np.ones((3, 3), np.uint8))
    # and each equals the reference's program of the same name, step by step
    el = R.element_set()["rect3x5"]
    for op in CR.MORPH_OPS:
        for border in CR.BORDERS:
            assert _shape(Morph(op, el, 2, border)) == _shape(to_chain(CR.morph(op, el, 2, border))), (op, border)


def test_a_chain_flattens_nested_chains_and_combines():
    t = Table(CR.threshold_table())
    c = Chain([Rank.median(3), Morph("gradient"), t])
    assert _shape(c) == [(STEP_RANK, 0, 0, 2), (STEP_RANK, 1, 0, 1), (STEP_RANK, 1, 0, 0), (STEP_BINARY, 2, 3, 0),
                         (STEP_TABLE, 4, 0, 0)]
    assert _shape(c) == _shape(to_chain(CR.program_set()["edges"]))
    g3, g5 = vfilter.kernels.gaussian3(), vfilter.kernels.gaussian5()
    dog = Chain([Combine("absdiff", Kernel(g3), Kernel(g5)), Table(CR.gamma_table())])
    assert _shape(dog) == [(STEP_CONV, 0, 0, 0), (STEP_CONV, 0, 0, 0), (STEP_BINARY, 1, 2, 2), (STEP_TABLE, 3, 0, 0)]
    diamond = Chain([Combine("add", Rank.erode(np.ones((7, 7))), None)])
    assert _shape(diamond) == [(STEP_RANK, 0, 0, 0), (STEP_BINARY, 1, 0, 1)]
    inv = Chain(Invert())
    assert _shape(inv) == [(STEP_TABLE, 0, 0, 0)] and inv.steps[0][4] == bytes(255 - v for v in range(256))
    assert inv.family == "chain" and inv.args == (inv.steps,)
    with pytest.raises(dataclasses.FrozenInstanceError):
        inv.steps = ()


def test_bad_programs_are_refused_with_the_reason():
    inv = Invert()
    with pytest.raises(ValueError, match="9 steps; at most 8"):
        Chain([inv] * 9)
    with pytest.raises(ValueError, match="9 steps; at most 8"):
        Chain.program([(inv, i) for i in range(9)])
    assert len(Chain([inv] * 8)) == 8
    with pytest.raises(ValueError, match="value 1 is read by no step"):
        Chain.program([(inv, 0), (inv, 0)])
    with pytest.raises(ValueError, match="value 2 is read by no step"):
        Chain.program([(inv, 0), (inv, 1), ("add", 1, 0)])
    with pytest.raises(ValueError, match="not an earlier value"):
        Chain.program([(inv, 1)])
    with pytest.raises(ValueError, match="not an earlier value"):
        Chain.program([(inv, 0), ("subtract", 1, 2)])  # reads itself
    with pytest.raises(ValueError, match="not a value"):
        Chain.program([(inv, -1)])
    with pytest.raises(ValueError, match="empty program"):
        Chain([])
    with pytest.raises(ValueError, match="op must be one of"):
        Combine("xor")
    with pytest.raises(ValueError, match="op must be one of"):
        Chain.program([("xor", 0, 0)])
    with pytest.raises(ValueError, match="not int"):
        Chain([3])
    with pytest.raises(ValueError, match="iterations=4 is a chain of 9 steps.*at most 8"):
        Morph("gradient", None, 4)
    with pytest.raises(ValueError, match="iterations=5 is a chain of 10 steps.*limited by that cap"):
        Morph("open", None, 5)
    assert len(Morph("erode", None, 8)) == 8 and len(Morph("close", None, 4)) == 8 and len(Morph("tophat", None, 3)) == 7
    with pytest.raises(ValueError, match="iterations must be a positive integer"):
        Morph("open", None, 0)
    with pytest.raises(ValueError, match="op must be one of"):
        Morph("hitmiss")
    # what the single-filter values refuse is refused when the step is built
    with pytest.raises(ValueError):
        Chain([Rank.erode(np.zeros((3, 3)))])
    with pytest.raises(ValueError):
        Morph("open", np.ones((2, 2)))


def test_a_three_channel_table_on_one_channel_frames_is_refused_before_any_gpu_work(monkeypatch):
    def no_context():
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(vfilter.filters, "get_context", no_context)
    c = to_chain(CR.program_set()["pointwise"])
    assert c.table_channels == 3
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 1), np.uint8)):
        with pytest.raises(ValueError, match="3-channel table"):
            vfilter.chain(bad, c)
        with pytest.raises(ValueError, match="3-channel table"):
            vfilter.chain_frames([bad], c)
    with pytest.raises(ValueError, match="uint8"):
        vfilter.chain(np.zeros((4, 5, 3), np.float32), c)
    with pytest.raises(ValueError, match="one channel count"):
        vfilter.chain_frames([np.zeros((2, 2), np.uint8), np.zeros((2, 2, 3), np.uint8)], Chain(Invert()))
    with pytest.raises(ValueError, match="iterations"):
        vfilter.morphology_ex(np.zeros((4, 5, 3), np.uint8), "gradient", None, 4)


def test_the_reference_equals_cv2_where_cv2_is_importable():
    cv2 = pytest.importorskip("cv2")
    codes = {"erode": cv2.MORPH_ERODE, "dilate": cv2.MORPH_DILATE, "open": cv2.MORPH_OPEN, "close": cv2.MORPH_CLOSE,
             "gradient": cv2.MORPH_GRADIENT, "tophat": cv2.MORPH_TOPHAT, "blackhat": cv2.MORPH_BLACKHAT}
    rng = np.random.default_rng(19)
    for shape in [(1, 1, 3), (6, 7, 3), (9, 4, 1), (17, 13, 3)]:
        f = rng.integers(0, 256, shape, dtype=np.uint8)
        for name in ("rect3", "cross5", "rect3x5", "random7"):
            e = R.element_set()[name]
            for op, code in codes.items():
                for it in (1, 2):
                    want = cv2.morphologyEx(f, code, e, iterations=it).reshape(shape)
                    assert np.array_equal(CR.run(f, CR.morph(op, e, it)), want), (shape, name, op, it)


def test_a_chain_copies_its_arrays_and_is_immutable():
    e = vfilter.elements.cross(5)
    t = CR.threshold_table().copy()
    c = Chain([Morph("gradient", e), Table(t)])
    e[:] = 0  # the caller's arrays may change at once
    t[:] = 0
    assert np.array_equal(c.steps[0][4], vfilter.elements.cross(5)) and c.steps[3][4] == CR.threshold_table().tobytes()
    with pytest.raises(ValueError):
        c.steps[0][4][0, 0] = 1
    with pytest.raises(Exception):
        c.steps[0] = None


def test_the_worker_command_line_refuses_bad_combinations_without_a_context(monkeypatch):
    from vfilter import chain_worker

    def no_worker(*a, **k):
        raise AssertionError("a worker was built")

    real = chain_worker.ChainWorker
    monkeypatch.setattr(chain_worker, "ChainWorker", no_worker)
    bad = [["--morph", "hitmiss"], ["--morph", "open", "--size", "4"], ["--morph", "open", "--size", "9"],
           ["--morph", "close", "--size", "3", "5", "7"], ["--morph", "gradient", "--iterations", "4"],
           ["--morph", "open", "--iterations", "0"], ["--morph", "erode", "--iterations", "9"],
           ["--morph", "open", "--element", "ellipse"], ["--morph", "open", "--border", "wrap"],
           ["--morph", "open", "--shape", "480", "480", "2"], []]
    for argv in bad:
        with pytest.raises((ValueError, SystemExit)):
            chain_worker.main(argv)
    good = chain_worker.morph_from_options("tophat", "cross", (3, 5), 2, "reflect101")
    assert _shape(good) == _shape(Morph("tophat", None, 2))
    assert np.array_equal(good.steps[0][4], vfilter.elements.cross(3, 5)) and good.steps[0][6] == 0
    assert chain_worker.morph_from_options("open").steps[0][6] == 2  # constant by default
    with pytest.raises(ValueError, match="limited by that cap"):
        chain_worker.morph_from_options("blackhat", iterations=4)
    with pytest.raises(ValueError):
        real("127.0.0.1", 1, 1, 0.0, chain=[Invert()])  # a Chain, not a list: refused before the worker's context
