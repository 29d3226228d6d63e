"""The numpy reference of filter chains for the chain tests: a program interpreter over
``_conv_ref.filter2d``, ``_rank_ref.apply`` and ``np.take``, with int16 arithmetic and a clip for
the binary ops.  A transcription of the definition in DESIGN.md 19; shares no code with ``vfilter``.

A program is a list of steps; value 0 is the frame and value i the result of step i (1-based):

    ("table", a, table)                     table: uint8 (256,) or (256, 3), cv2.LUT's
    ("conv", a, weights, shift, border)     _conv_ref.filter2d's arguments
    ("rank", a, op, arg, border)            _rank_ref.apply's: op "erode" / "dilate" with an element,
                                            "median" with a ksize
    ("bin", op, a, b)                       op "subtract", "add", "absdiff", "min", "max"

The result is the last step's value; every step sees the whole frame."""
import numpy as np

import _conv_ref
import _rank_ref

BORDERS = _rank_ref.BORDERS
MAX_STEPS = 8
MORPH_OPS = ("erode", "dilate", "open", "close", "gradient", "tophat", "blackhat")


def binary(op, a, b):
    x, y = a.astype(np.int16), b.astype(np.int16)
    r = {"subtract": lambda: x - y, "add": lambda: x + y, "absdiff": lambda: np.abs(x - y),
         "min": lambda: np.minimum(x, y), "max": lambda: np.maximum(x, y)}[op]()
    return np.clip(r, 0, 255).astype(np.uint8)


def table(img, t):
    t = np.asarray(t)
    assert t.dtype == np.uint8
    if t.shape == (256,):
        return np.take(t, img)
    assert t.shape == (256, 3) and img.ndim == 3 and img.shape[2] == 3
    return np.stack([np.take(t[:, c], img[:, :, c]) for c in range(3)], axis=2)


def run(img, prog):
    """The program's result on the whole frame ``img`` (uint8 H x W or H x W x C)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and 1 <= len(prog) <= MAX_STEPS
    vals = [img]
    for st in prog:
        if st[0] == "table":
            out = table(vals[st[1]], st[2])
        elif st[0] == "conv":
            out = _conv_ref.filter2d(vals[st[1]], st[2], st[3], st[4])
        elif st[0] == "rank":
            out = _rank_ref.apply(vals[st[1]], st[2], st[3], st[4])
        else:
            assert st[0] == "bin"
            out = binary(st[1], vals[st[2]], vals[st[3]])
        assert out.shape == img.shape and out.dtype == np.uint8
        vals.append(out)
    return vals[-1]


def morph(op, element, iterations=1, border="constant"):
    """The program of ``morphology_ex(src, op, element, iterations, border)``: with E^n / D^n for n
    successive erosions / dilations, erode E^n, dilate D^n, open D^n(E^n x), close E^n(D^n x),
    gradient subtract(D^n x, E^n x), tophat subtract(x, open), blackhat subtract(close, x)."""
    n = iterations
    prog = []

    def rep(kind, v):
        for _ in range(n):
            prog.append(("rank", v, kind, element, border))
            v = len(prog)
        return v

    if op in ("erode", "dilate"):
        rep(op, 0)
    elif op == "open":
        rep("dilate", rep("erode", 0))
    elif op == "close":
        rep("erode", rep("dilate", 0))
    elif op == "gradient":
        d = rep("dilate", 0)
        e = rep("erode", 0)
        prog.append(("bin", "subtract", d, e))
    elif op == "tophat":
        o = rep("dilate", rep("erode", 0))
        prog.append(("bin", "subtract", 0, o))
    else:
        assert op == "blackhat"
        c = rep("erode", rep("dilate", 0))
        prog.append(("bin", "subtract", c, 0))
    return prog


def moved(prog, base, src):
    """``prog`` as part of a longer program: its value 0 is value ``src``, its value i is base + i."""
    def v(x):
        return src if x == 0 else base + x
    out = []
    for st in prog:
        if st[0] == "bin":
            out.append(("bin", st[1], v(st[2]), v(st[3])))
        else:
            out.append((st[0], v(st[1])) + tuple(st[2:]))
    return out


def gamma_table(g=0.5):
    return np.clip(np.rint(255.0 * (np.arange(256) / 255.0) ** g), 0, 255).astype(np.uint8)


def threshold_table(t=24):
    return np.where(np.arange(256) > t, 255, 0).astype(np.uint8)


def curves_table():
    """Three different curves, one per channel: (256, 3)."""
    v = np.arange(256)
    return np.stack([gamma_table(0.7), (255 - v).astype(np.uint8), np.clip(2 * v - 64, 0, 255).astype(np.uint8)], axis=1)


INVERT = (255 - np.arange(256)).astype(np.uint8)


def program_set(border="constant", channels=3):
    """The programs the tests use, by name.  ``border`` goes to every erode / dilate / conv step (the
    median replicates, always); with ``channels`` 1 ``pointwise`` takes a one-channel curve (a
    3-channel table on a 1-channel frame is invalid)."""
    el = _rank_ref.element_set()
    ks = _conv_ref.kernel_set()
    g3, g5 = ks["gaussian3"], ks["gaussian5"]
    curves = curves_table() if channels == 3 else gamma_table(0.7)
    edges = [("rank", 0, "median", 3, "replicate")] + moved(morph("gradient", el["rect3"], 1, border), 1, 1)
    edges.append(("table", len(edges), threshold_table()))
    eight = [
        ("rank", 0, "erode", el["rect3"], border),          # 1
        ("rank", 1, "dilate", el["rect3"], border),         # 2
        ("bin", "subtract", 0, 2),                          # 3: a top-hat
        ("table", 3, gamma_table(0.5)),                     # 4
        ("conv", 4, g3[0], g3[1], border),                  # 5
        ("rank", 5, "median", 3, "replicate"),              # 6
        ("bin", "max", 6, 1),                               # 7
        ("bin", "add", 7, 3),                               # 8
    ]
    return {
        "open3": morph("open", el["rect3"], 1, border),
        "close_cross5": morph("close", el["cross5"], 1, border),
        "gradient_random7": morph("gradient", el["random7"], 1, border),
        "gradient_corner5": morph("gradient", el["corner5"], 1, border),
        # corner5 has one member, so erode == dilate wherever the set is not empty and the gradient is
        # 0 there; where it is empty (the top and left edges under "constant") erode gives 255 and
        # dilate 0: the gradient saturates to 0 as well, the reversed subtraction gives 255
        "corner5_reversed": morph("gradient", el["corner5"], 1, border)[:2] + [("bin", "subtract", 2, 1)],
        "tophat3x5": morph("tophat", el["rect3x5"], 1, border),
        "blackhat3_it2": morph("blackhat", el["rect3"], 2, border),
        "edges": edges,
        "dog": [("conv", 0, g3[0], g3[1], border), ("conv", 0, g5[0], g5[1], border), ("bin", "absdiff", 1, 2),
                ("table", 3, gamma_table(0.5))],
        "pointwise": [("table", 0, INVERT), ("table", 1, curves), ("table", 2, INVERT)],
        "diamond": [("rank", 0, "erode", el["rect7"], border), ("bin", "add", 1, 0)],
        "eight": eight,
    }


def reach(prog):
    """The largest summed vertical radius along a path from the result to value 0."""
    n = len(prog)
    r = [-1] * (n + 1)
    r[n] = 0
    for i in range(n, 0, -1):
        st = prog[i - 1]
        if r[i] < 0:
            continue
        if st[0] == "conv":
            ops, rad = [st[1]], np.asarray(st[2]).shape[0] // 2
        elif st[0] == "rank":
            ops, rad = [st[1]], (st[3] if st[2] == "median" else np.asarray(st[3]).shape[0]) // 2
        elif st[0] == "table":
            ops, rad = [st[1]], 0
        else:
            ops, rad = [st[2], st[3]], 0
        for a in ops:
            r[a] = max(r[a], r[i] + rad)
    return r[0]


def noise(h, w, c=3, seed=0):
    shape = (h, w) if c == 1 else (h, w, c)
    return np.random.default_rng([h, w, c, seed]).integers(0, 256, shape, dtype=np.uint8)
