"""The rank filters on the CPU: the numpy reference of ``tests/_rank_ref.py`` against a plain
triple loop over the definition, so the reference the GPU tests compare with is
itself guarded; ``vfilter.elements`` against their definitions; what ``as_element``, ``Rank`` and
the ``RankWorker`` command line refuse, all before any GPU work.  Where ``cv2`` is importable the
reference is also compared with it (skipped otherwise)."""
import numpy as np
import pytest

import _rank_ref as R
import vfilter
from vfilter import elements, rank_worker
from vfilter.filters import Rank

ELEMENTS = R.element_set()


def _bidx(p, n, border):
    """The index tap position p reads on an axis of n, or None when the tap is left out."""
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


def _loop(src, op, arg, border):
    h, w, ch = src.shape
    e = np.ones((arg, arg), np.uint8) if op == "median" else arg
    kh, kw = e.shape
    out = np.empty_like(src)
    for y in range(h):
        for x in range(w):
            for c in range(ch):
                s = []
                for j in range(kh):
                    for i in range(kw):
                        if not e[j, i]:
                            continue
                        by, bx = _bidx(y + j - kh // 2, h, border), _bidx(x + i - kw // 2, w, border)
                        if by is not None and bx is not None:
                            s.append(int(src[by, bx, c]))
                if op == "erode":
                    out[y, x, c] = min(s) if s else 255
                elif op == "dilate":
                    out[y, x, c] = max(s) if s else 0
                else:
                    assert len(s) == arg * arg
                    out[y, x, c] = sorted(s)[len(s) // 2]
    return out


def _frames():
    rng = np.random.default_rng(11)
    shapes = [(1, 1, 3), (1, 5, 1), (2, 2, 3), (6, 7, 3), (5, 1, 1), (3, 4, 3)]
    out = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    out.append(rng.choice(np.array([0, 1, 2, 3, 252, 253, 254, 255], np.uint8), (6, 7, 3)))  # ties and both extremes
    return out


@pytest.mark.parametrize("border", R.BORDERS)
@pytest.mark.parametrize("name", list(ELEMENTS))
@pytest.mark.parametrize("op", ["erode", "dilate"])
def test_morphology_reference_against_the_triple_loop(op, name, border):
    for f in _frames():
        got = R.apply(f, op, ELEMENTS[name], border)
        assert got.dtype == np.uint8 and np.array_equal(got, _loop(f, op, ELEMENTS[name], border)), (f.shape, name)


@pytest.mark.parametrize("ksize", [3, 5])
def test_median_reference_against_the_triple_loop(ksize):
    for f in _frames():
        assert np.array_equal(R.median(f, ksize), _loop(f, "median", ksize, "replicate")), f.shape
    flat = _frames()[3][:, :, 0].copy()
    assert np.array_equal(R.median(flat, ksize), R.median(flat[:, :, None], ksize)[:, :, 0])


def test_the_empty_set_and_the_off_centre_members():
    """corner5's one member is 2 up and 2 left: under the constant border the first two rows and
    columns have no tap in the frame (255 for erode, 0 for dilate); elsewhere the result is the
    frame shifted, so a flipped or transposed element cannot pass."""
    f = _frames()[3]
    c5 = ELEMENTS["corner5"]
    er, di = R.erode(f, c5), R.dilate(f, c5)
    assert (er[:2] == 255).all() and (er[:, :2] == 255).all() and (di[:2] == 0).all() and (di[:, :2] == 0).all()
    assert np.array_equal(er[2:, 2:], f[:-2, :-2]) and np.array_equal(di[2:, 2:], f[:-2, :-2])
    assert np.array_equal(R.erode(f, np.ones((1, 1), np.uint8)), f)


def test_elements_against_their_definitions():
    for w in (1, 3, 5, 7):
        for h in (1, 3, 5, 7):
            r, c = elements.rect(w, h), elements.cross(w, h)
            assert r.shape == c.shape == (h, w) and r.dtype == c.dtype == np.uint8
            assert (r == 1).all()
            want = np.array([[1 if (j == h // 2 or i == w // 2) else 0 for i in range(w)] for j in range(h)], np.uint8)
            assert np.array_equal(c, want)
            assert np.array_equal(r, R.rect(w, h)) and np.array_equal(c, R.cross(w, h))
        assert np.array_equal(elements.rect(w), elements.rect(w, w)) and np.array_equal(elements.cross(w), elements.cross(w, w))
    for bad in [(2,), (0,), (9,), (3, 4), (3, 9), (-3,), (3.5,)]:
        with pytest.raises(ValueError):
            elements.rect(*bad)
        with pytest.raises(ValueError):
            elements.cross(*bad)


def test_as_element_and_rank_refusals():
    assert np.array_equal(vfilter.as_element(None), np.ones((3, 3), np.uint8))
    e = vfilter.as_element(np.array([[0, 7, 0], [2, 0, -1], [0, 1.0, 0]]))
    assert e.dtype == np.uint8 and e.flags.c_contiguous and np.array_equal(e, [[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    assert np.array_equal(vfilter.as_element(np.array([[True, False, True]])), [[1, 0, 1]])
    bad = [np.ones((2, 3)), np.ones((3, 4), int), np.ones((9, 9), np.uint8), np.zeros((3, 3), np.uint8),
           np.ones((3, 3, 3), np.uint8), np.ones(3, np.uint8), np.full((3, 3), 0.5), np.array([["a"]]), np.ones((0, 3))]
    for b in bad:
        with pytest.raises(ValueError):
            vfilter.as_element(b)
        for make in (Rank.erode, Rank.dilate):
            with pytest.raises(ValueError):
                make(b)
    for k in (1, 4, 7, 0, -3, 3.0, "3", None, True):
        with pytest.raises(ValueError):
            Rank.median(k)
    for border in ("wrap", None, 0, "reflect"):
        with pytest.raises(ValueError):
            Rank.erode(None, border)
        with pytest.raises(ValueError):
            Rank.dilate(elements.cross(3), border)
    with pytest.raises(ValueError):
        Rank("open", None)
    with pytest.raises(ValueError):
        Rank("median", elements.cross(3), "replicate")
    with pytest.raises(ValueError):
        Rank("median", elements.rect(3), "constant")
    with pytest.raises(ValueError):
        Rank("median", elements.rect(7), "replicate")
    # the frame checks of the drop-ins come before any GPU work too
    for fn in (vfilter.erode, vfilter.dilate):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4, 3), np.float32))
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4, 3), np.uint8), np.ones((2, 2)))
    with pytest.raises(ValueError):
        vfilter.median_blur(np.zeros((4, 4, 3), np.uint8), 7)
    with pytest.raises(ValueError):
        vfilter.rank_frames([np.zeros((4, 4, 3), np.uint8)], "median")


def test_rank_is_immutable_and_copies_its_element():
    e = elements.cross(5)
    r = Rank.dilate(e, "replicate")
    e[:] = 0  # the caller's array may change at once
    assert np.array_equal(r.element, elements.cross(5))
    assert (r.family, r.op, r.op_code, r.border, r.border_code) == ("rank", "dilate", 1, "replicate", 1)
    op, el, border = r.args
    assert (op, border) == (1, 1) and el is r.element and el.dtype == np.uint8 and el.flags.c_contiguous
    with pytest.raises(ValueError):
        r.element[0, 0] = 1
    with pytest.raises(Exception):
        r.border = "constant"
    with pytest.raises(Exception):
        r.element = e
    d = Rank.erode()
    assert d.args[0] == 0 and d.args[2] == 2 and np.array_equal(d.element, np.ones((3, 3), np.uint8))  # constant by default
    m = Rank.median(5)
    assert m.args[0] == 2 and m.args[2] == 1 and m.element.shape == (5, 5) and m.element.all() and m.border == "replicate"


def test_the_worker_command_line_refuses_bad_combinations_without_a_context(monkeypatch):
    def no_worker(*a, **k):
        raise AssertionError("a worker was built")

    monkeypatch.setattr(rank_worker, "RankWorker", no_worker)
    bad = [["--op", "median", "--element", "cross"], ["--op", "median", "--size", "7"], ["--op", "median", "--size", "3", "5"],
           ["--op", "median", "--size", "4"], ["--op", "median", "--border", "constant"], ["--op", "erode", "--size", "4"],
           ["--op", "erode", "--size", "9"], ["--op", "dilate", "--size", "3", "5", "7"], ["--op", "erode", "--shape", "480", "480", "2"],
           ["--op", "open"], ["--op", "erode", "--element", "ellipse"], ["--op", "erode", "--border", "wrap"], []]
    for argv in bad:
        with pytest.raises((ValueError, SystemExit)):
            rank_worker.main(argv)
    good = rank_worker.rank_from_options("erode", "cross", (3, 5), "reflect101")
    assert np.array_equal(good.element, elements.cross(3, 5)) and good.args[0] == 0 and good.border == "reflect101"
    assert rank_worker.rank_from_options("dilate").border == "constant"
    m = rank_worker.rank_from_options("median", "rect", (5,))
    assert m.op == "median" and m.element.shape == (5, 5) and m.border == "replicate"


def test_the_reference_equals_cv2_where_cv2_is_importable():
    cv2 = pytest.importorskip("cv2")
    for f in _frames():
        f = np.ascontiguousarray(f)
        for name, e in ELEMENTS.items():
            assert np.array_equal(R.erode(f, e).reshape(f.shape), cv2.erode(f, e).reshape(f.shape)), name
            assert np.array_equal(R.dilate(f, e).reshape(f.shape), cv2.dilate(f, e).reshape(f.shape)), name
        for k in (3, 5):
            assert np.array_equal(R.median(f, k).reshape(f.shape), cv2.medianBlur(f, k).reshape(f.shape))
    for w, h in [(3, 3), (5, 3), (3, 7), (7, 7)]:
        assert np.array_equal(elements.rect(w, h), cv2.getStructuringElement(cv2.MORPH_RECT, (w, h)))
        assert np.array_equal(elements.cross(w, h), cv2.getStructuringElement(cv2.MORPH_CROSS, (w, h)))
