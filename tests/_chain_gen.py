"""A seeded generator of valid filter-chain programs, in the tuple format of ``tests/_chain_ref.py``
(so ``_chain_ref.run`` is their reference and ``_chain_build.to_chain`` builds their ``Chain``).
Shares no code with ``vfilter``.

``generate(seed, channels)`` draws one program of 1 to 8 steps:

    table   a random permutation of 0..255, (256,) or -- for 3-channel frames -- (256, 3): a
            permutation keeps every value of the picture apart (a threshold would collapse it)
    conv    kh and kw drawn independently from 1, 3, 5, 7; small signed weights with the centre set
            so that sum K == 2^shift (unit gain), shift 0 .. 8; one draw in four has large weights,
            so that both arithmetic forms (sum|K| <= 128 and above) occur; its own border
    rank    erode / dilate over a random 0/1 element with independent odd sides 1 .. 7 and at least
            one member, its own border; or the median 3 / 5 (replicate)
    bin     all five ops; operands prefer values no step has read yet; a == b for add, min and max
            only (subtract(x, x) and absdiff(x, x) are identically 0)

Every value but the last is read (``validate()``'s dead-value rule): the draw of a step's operands is
steered so that the steps still to come can read what is left.

``PROGRAMS`` / ``PROGRAMS_1``: name -> program for 3-channel / 1-channel frames, 64 generated ones
and the hand-written ``extra()`` for what a draw may miss.  ``features(prog)`` names what a program
holds, from its text alone; ``tests/test_chain_gen.py`` asserts that the set holds every feature.
"""
import numpy as np

import _chain_ref as CR

SIDES = (1, 3, 5, 7)
BIN_OPS = ("subtract", "add", "absdiff", "min", "max")
SAME_OPERAND_OPS = ("add", "min", "max")
N_GENERATED = 64
_LENGTH_P = np.array([0.12, 0.14, 0.14, 0.14, 0.14, 0.13, 0.11, 0.08])  # 1 .. 8 steps


def permutation(rng, channels=1):
    if channels == 1:
        return rng.permutation(256).astype(np.uint8)
    return np.stack([rng.permutation(256) for _ in range(3)], axis=1).astype(np.uint8)


def unit_gain_kernel(rng, kh, kw, shift, big):
    """kh x kw signed weights with sum K == 2^shift: the centre takes what the others leave."""
    m = int(rng.integers(8, 41)) if big else int(rng.integers(1, 4))
    k = rng.integers(-m, m + 1, (kh, kw)).astype(np.int64)
    k[kh // 2, kw // 2] = 0
    k[kh // 2, kw // 2] = (1 << shift) - int(k.sum())
    assert int(k.sum()) == 1 << shift
    return k


def random_element(rng, kh, kw):
    e = (rng.integers(0, 2, (kh, kw)) != 0).astype(np.uint8)
    if not e.any():
        e[int(rng.integers(kh)), int(rng.integers(kw))] = 1
    return e


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def generate(seed, channels=3):
    rng = np.random.default_rng([seed, channels])
    n = int(rng.choice(np.arange(1, CR.MAX_STEPS + 1), p=_LENGTH_P))
    prog = []
    unread = [0]
    for i in range(1, n + 1):
        rem = n - i  # the steps after this one; each can take the count of unread values down by one
        must = max(0, len(unread) - rem)  # the unread values this step has to read
        assert must <= 2
        kind = "bin" if must == 2 else _pick(rng, ("table", "conv", "conv", "rank", "rank", "bin"))

        def operand(avoid=None):
            fresh = [v for v in unread if v != avoid]
            if fresh and (must or rng.random() < 0.7):
                return int(_pick(rng, fresh))
            return int(rng.integers(i))

        a = operand()
        if kind == "table":
            st = ("table", a, permutation(rng, 3 if channels == 3 and rng.random() < 0.5 else 1))
        elif kind == "conv":
            kh, kw = int(_pick(rng, SIDES)), int(_pick(rng, SIDES))
            shift = int(rng.integers(0, 9))
            st = ("conv", a, unit_gain_kernel(rng, kh, kw, shift, rng.random() < 0.25), shift, _pick(rng, CR.BORDERS))
        elif kind == "rank":
            if rng.random() < 0.25:
                st = ("rank", a, "median", int(_pick(rng, (3, 5))), "replicate")
            else:
                kh, kw = int(_pick(rng, SIDES)), int(_pick(rng, SIDES))
                st = ("rank", a, _pick(rng, ("erode", "dilate")), random_element(rng, kh, kw), _pick(rng, CR.BORDERS))
        else:
            same = must < 2 and (i == 1 or rng.random() < 0.3)
            if same:
                st = ("bin", _pick(rng, SAME_OPERAND_OPS), a, a)
            else:
                b = operand(avoid=a)
                while b == a:
                    b = int(rng.integers(i))
                if must == 2:
                    assert a in unread and b in unread
                st = ("bin", _pick(rng, BIN_OPS), a, b) if rng.random() < 0.5 else ("bin", _pick(rng, BIN_OPS), b, a)
        prog.append(st)
        for v in (st[2], st[3]) if st[0] == "bin" else (st[1],):
            if v in unread:
                unread.remove(v)
        unread.append(i)
    assert unread == [n], (seed, channels, unread)
    return prog


def extra(channels=3):
    """Hand-written programs for the features a draw may miss (tests/test_chain_gen.py names them)."""
    rng = np.random.default_rng([99, channels])
    t = [permutation(rng) for _ in range(3)]
    t3 = permutation(rng, 3) if channels == 3 else permutation(rng)
    row7 = unit_gain_kernel(rng, 1, 7, 5, False)
    col7 = unit_gain_kernel(rng, 7, 1, 5, False)
    e17, e71, e35 = random_element(rng, 1, 7), random_element(rng, 7, 1), random_element(rng, 3, 5)
    return {
        # value 1 (a table) is read by steps 2 and 3: it is not folded
        "x_table_two_readers": [("table", 0, t[0]), ("rank", 1, "erode", e35, "reflect101"), ("bin", "subtract", 1, 2)],
        # tables in sequence fold: 3 channels then 1, and after the neighbourhood step two of 1
        "x_tables_fold": [("table", 0, t3), ("table", 1, t[0]), ("conv", 2, row7, 5, "replicate"), ("table", 3, t[1]),
                          ("table", 4, t[2])],
        # subtract(a = 1, b = 2): b dies here, a is read by step 4: in place over b, not commutative
        "x_subtract_over_b": [("rank", 0, "dilate", e17, "constant"), ("rank", 0, "erode", e71, "constant"),
                              ("bin", "subtract", 1, 2), ("bin", "max", 3, 1)],
        # separable: 1 x 7 then 7 x 1; value 0 is dead at step 2, so the result lands in buffer 0
        "x_separable": [("conv", 0, row7, 5, "reflect101"), ("conv", 1, col7, 5, "constant")],
        "x_separable_rank": [("rank", 0, "erode", np.ones((1, 7), np.uint8), "replicate"),
                             ("rank", 1, "erode", np.ones((7, 1), np.uint8), "reflect101")],
        # two neighbourhood readers of value 1 with different kh, the last step a table
        "x_two_readers": [("rank", 0, "median", 3, "replicate"), ("conv", 1, col7, 5, "reflect101"),
                          ("rank", 1, "dilate", e17, "replicate"), ("bin", "absdiff", 2, 3), ("table", 4, t[0])],
    }


def _build(channels):
    out = {"g%02d" % s: generate(s, channels) for s in range(N_GENERATED)}
    out.update(extra(channels))
    return out


PROGRAMS = _build(3)
PROGRAMS_1 = _build(1)
GENERATED = sorted(n for n in PROGRAMS if n.startswith("g"))


def sides(st):
    """(kh, kw) of a neighbourhood step, None for the others."""
    if st[0] == "conv":
        return tuple(np.asarray(st[2]).shape)
    if st[0] == "rank":
        return (st[3], st[3]) if st[2] == "median" else tuple(np.asarray(st[3]).shape)
    return None


def operands(st):
    return (st[2], st[3]) if st[0] == "bin" else (st[1],)


def readers(prog, v):
    return [i for i, st in enumerate(prog, 1) if v in operands(st)]


def features(prog):
    """The named features of the issue that ``prog`` holds, from its text alone (those that need the
    plan -- buffers, folding -- are ``tests/test_chain_gen.py``'s, from the checker)."""
    f = set()
    n = len(prog)
    nb = [st for st in prog if sides(st)]
    if any(st[0] == "bin" and st[2] == st[3] for st in prog):
        f.add("same_operand")
    for v in range(n):
        rd = [prog[i - 1] for i in readers(prog, v)]
        if len(rd) >= 2 and any(sides(st) for st in rd):
            f.add("shared_with_neighbourhood")
        if len({sides(st)[0] for st in rd if sides(st)}) >= 2:
            f.add("two_neighbourhood_readers_of_different_kh")
        if v and prog[v - 1][0] == "table" and len(rd) >= 2:
            f.add("table_with_two_readers")
        if v and prog[v - 1][0] == "table" and len(rd) == 1 and rd[0][0] == "table":
            f.add("tables_fold")
            if np.asarray(prog[v - 1][2]).ndim == 2 and np.asarray(rd[0][2]).ndim == 1:
                f.add("tables_fold_3_then_1")
    for st in nb:
        kh, kw = sides(st)
        if kw > kh:
            f.add("wider_than_tall")
        if kh > kw:
            f.add("taller_than_wide")
        if kh == 1 < kw:
            f.add("one_row")
    borders = {st[4] for st in nb}
    if len(borders) >= 2:
        f.add("mixed_borders")
    if nb and CR.reach(prog) == 0:
        f.add("neighbourhood_without_reach")
    for st in prog:
        if st[0] == "conv":
            f.add("narrow_form" if int(np.abs(np.asarray(st[2])).sum()) <= 128 else "wide_form")
        if st[0] == "bin":
            f.add("op_" + st[1])
    f.add("length_%d" % n)
    f.add("ends_with_" + ("neighbourhood" if sides(prog[-1]) else prog[-1][0]))
    return f


def serialise(progs, channels):
    """The structure of programs as the text ``chain_plan_check plan`` reads: per program a line
    ``P <steps> <channels>`` and per step ``<kind> <a> <b> <op> <kw> <kh> <table channels>``."""
    kinds = {"table": 0, "conv": 1, "rank": 2, "bin": 3}
    lines = []
    for prog in progs:
        lines.append("P %d %d" % (len(prog), channels))
        for st in prog:
            a, b = (st[2], st[3]) if st[0] == "bin" else (st[1], 0)
            op = BIN_OPS.index(st[1]) if st[0] == "bin" else ("erode", "dilate", "median").index(st[2]) if st[0] == "rank" else 0
            kh, kw = sides(st) or (0, 0)
            tch = 3 if st[0] == "table" and np.asarray(st[2]).ndim == 2 else 1
            lines.append("%d %d %d %d %d %d %d" % (kinds[st[0]], a, b, op, kw, kh, tch))
    return "\n".join(lines) + "\n"
