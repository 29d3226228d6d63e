"""``tests/_chain_ref.py``'s interpreter extended by the separable step, without editing it:

    ("sep", a, kx, ky, shift, divisor, rounding, border)      _sep_ref.sep's arguments

Every other step is handed to ``_chain_ref``.  ``generate(seed)`` draws a ``tests/_chain_gen.py``
program for 3-channel frames and puts a random separable filter in the place of every convolution
step (of its last step that is not binary, or of a step appended, when it has none).  Shares no
code with ``vfilter``.
"""
import numpy as np

import _chain_gen as G
import _chain_ref as CR
import _sep_ref as S

ROUNDINGS = ("half_even", "half_up")
BORDERS = ("reflect101", "replicate", "constant")


def run(img, prog):
    """The program's result on the whole frame ``img`` (uint8 H x W or H x W x C)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and 1 <= len(prog) <= CR.MAX_STEPS
    vals = [img]
    for st in prog:
        if st[0] == "sep":
            out = S.sep(vals[st[1]], *st[2:])
        elif st[0] == "bin":
            out = CR.binary(st[1], vals[st[2]], vals[st[3]])
        else:  # a one-step program on the operand
            out = CR.run(vals[st[1]], [(st[0], 0) + tuple(st[2:])])
        assert out.shape == img.shape and out.dtype == np.uint8
        vals.append(out)
    return vals[-1]


def reach(prog):
    """``_chain_ref.reach``: a sep step has the vertical radius of a len(ky) x 1 convolution."""
    return CR.reach([("conv", st[1], np.zeros((len(st[3]), 1)), 0, st[7]) if st[0] == "sep" else st for st in prog])


def random_sep(rng):
    """(kx, ky, shift, divisor, rounding, border): one in three a box with its divisor, else signed taps
    of unit gain (the centre takes what the others leave) with a shift; tap counts odd, up to 31."""
    kw, kh = (int(2 * rng.integers(0, 16) + 1) for _ in range(2))
    border = BORDERS[int(rng.integers(3))]
    if rng.random() < 1 / 3:
        return np.ones(kw, np.int64), np.ones(kh, np.int64), 0, kw * kh, "half_even", border
    taps, bits = [], []
    for n in (kw, kh):
        b = int(rng.integers(3, 8))
        k = rng.integers(-2, 3, n).astype(np.int64)
        k[n // 2] += (1 << b) - k.sum()
        taps.append(k)
        bits.append(b)
    assert np.abs(taps[0]).sum() * np.abs(taps[1]).sum() <= 65536
    return taps[0], taps[1], bits[0] + bits[1], 1, ROUNDINGS[int(rng.integers(2))], border


def generate(seed):
    """A program with at least one sep step, or None when the draw cannot hold one."""
    rng = np.random.default_rng([seed, 2107])
    prog = list(G.generate(seed, 3))
    at = [i for i, st in enumerate(prog) if st[0] == "conv"]
    if not at and len(prog) < CR.MAX_STEPS:
        prog.append(("conv", len(prog), None, 0, None))
        at = [len(prog) - 1]
    if not at:
        at = [i for i, st in enumerate(prog) if st[0] != "bin"][-1:]
    if not at:
        return None
    for i in at:
        prog[i] = ("sep", prog[i][1]) + random_sep(rng)
    return prog


def programs(count=32):
    """name -> program: the first ``count`` seeds that hold a sep step."""
    out, seed = {}, 0
    while len(out) < count:
        p = generate(seed)
        if p is not None:
            out["s%02d" % seed] = p
        seed += 1
    return out


def cost(prog):
    """What the numpy reference pays for a program, roughly: passes per pixel (a 5 x 5 median sorts)."""
    total = 0
    for st in prog:
        if st[0] == "sep":
            total += len(st[2]) + len(st[3])
            continue
        s = G.sides(st)
        total += 1 if s is None else s[0] * s[1] * (4 if st[0] == "rank" and st[2] == "median" else 1)
    return total
