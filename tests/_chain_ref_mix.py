"""``tests/_chain_ref.py``'s interpreter extended by the colour-matrix step, without editing it:

    ("mix", a, m, shift, rounding)          _mix_ref.mix's arguments: m the 3 x 4 int [M | t]

Every other step is handed to ``_chain_ref``.  ``generate(seed)`` draws a ``tests/_chain_gen.py``
program for 3-channel frames and puts a random colour matrix in the place of every table step (of its
last step that is not binary, or of a step appended, when it has no table).  Shares no code with ``vfilter``.
"""
import numpy as np

import _chain_gen as G
import _chain_ref as CR
import _mix_ref as M

ROUNDINGS = ("half_even", "half_up")


def run(img, prog):
    """The program's result on the whole frame ``img`` (uint8 H x W x 3)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and 1 <= len(prog) <= CR.MAX_STEPS
    vals = [img]
    for st in prog:
        if st[0] == "mix":
            out = M.mix(vals[st[1]], st[2], st[3], st[4])
        elif st[0] == "bin":
            out = CR.binary(st[1], vals[st[2]], vals[st[3]])
        else:  # a one-step program on the operand
            out = CR.run(vals[st[1]], [(st[0], 0) + tuple(st[2:])])
        assert out.shape == img.shape and out.dtype == np.uint8
        vals.append(out)
    return vals[-1]


def reach(prog):
    """``_chain_ref.reach``: a mix step has radius 0, as a table step has."""
    return CR.reach([("table", st[1], None) if st[0] == "mix" else st for st in prog])


def random_matrix(rng):
    """(3 x 4 int64, shift, rounding): small signed weights plus 2^shift on one input per row (so the
    picture survives), offsets of up to 40 grey levels; sum|M[c]| <= 65536 and |t| <= 255 * 2^shift hold."""
    shift = int(rng.integers(1, 15)) if rng.random() < 0.8 else 0  # one in five has nothing to round
    m = np.zeros((3, 4), np.int64)
    m[:, :3] = rng.integers(-(1 << shift) // 2, (1 << shift) // 2 + 1, (3, 3))
    for c in range(3):
        m[c, int(rng.integers(3))] += 1 << shift
    m[:, 3] = rng.integers(-40 << shift, (40 << shift) + 1, 3)
    assert np.abs(m[:, :3]).sum(axis=1).max() <= 65536 and np.abs(m[:, :3]).max() <= 32767
    return m, shift, ROUNDINGS[int(rng.integers(2))]


def generate(seed):
    """A program with at least one mix step, or None when the draw cannot hold one."""
    rng = np.random.default_rng([seed, 2005])
    prog = list(G.generate(seed, 3))
    at = [i for i, st in enumerate(prog) if st[0] == "table"]
    if not at and len(prog) < CR.MAX_STEPS:
        prog.append(("table", len(prog), None))
        at = [len(prog) - 1]
    if not at:
        at = [i for i, st in enumerate(prog) if st[0] != "bin"][-1:]
    if not at:
        return None
    for i in at:
        prog[i] = ("mix", prog[i][1]) + random_matrix(rng)
    return prog


def programs(count=32):
    """name -> program: the first ``count`` seeds that hold a mix step."""
    out, seed = {}, 0
    while len(out) < count:
        p = generate(seed)
        if p is not None:
            out["m%02d" % seed] = p
        seed += 1
    return out


def cost(prog):
    """What the numpy reference pays for a program, roughly: taps per pixel (a 5 x 5 median sorts)."""
    total = 0
    for st in prog:
        s = G.sides(st) if st[0] != "mix" else None
        total += 1 if s is None else s[0] * s[1] * (4 if st[0] == "rank" and st[2] == "median" else 1)
    return total
