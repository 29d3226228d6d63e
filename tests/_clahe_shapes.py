"""The CLAHE frames that are chosen by the loop they reach, and ``launch_all``'s arithmetic (``csrc/vf_clahe.hip``)
restated in Python: how many row slices the histogram cuts a tile into, how many ``kRows`` rounds a slice takes,
how many passes of ``kBlock`` lanes a tile row or a cell row takes, and how the blend cuts a cell into strips.
``tests/test_gpu_clahe_shapes.py`` asserts what the frames reach and runs them at the default switches;
``tests/_variant_cases.py`` runs them again under the read-once switches.  Nothing here needs a GPU."""
import collections
import os
import re

import numpy as np

import _clahe_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-video-filter_amd", "csrc")

# the values this arithmetic was written for; constants_in_the_sources() reads what the sources say today
K_BLOCK, K_ROWS, HIST_TARGET, APPLY_TARGET, REPLICAS = 256, 4, 1024, 512, 8

# name -> (height, width, (tiles_x, tiles_y))
CASES = {
    "a": (40, 520, (2, 2)),      # tiles 260 wide: 2 passes on one channel, 4 on three; 20 strips over cells of 10 rows
    "b": (330, 61, (16, 16)),    # slices of 6 rows (rounds of 4 and 2), a last slice of 3; two strips cut 21 rows unevenly
    "c": (586, 715, (8, 16)),    # slices of 5 rows, a last slice of 2; 270 row bytes on three channels: a second pass
    "d": (560, 48, (16, 16)),    # slices of 9 rows: rounds of 4, 4 and 1, the pattern of 1080p under 8 x 8
}


def constants_in_the_sources():
    """``(kBlock, kRows, kHistTarget, kApplyTarget, kClaheReplicas)`` as the sources define them."""
    text = open(os.path.join(CSRC, "vf_clahe.hip")).read() + open(os.path.join(CSRC, "vf_internal.h")).read()

    def value(name):
        found = re.findall(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(found) == 1, (name, found)
        return int(found[0])

    return tuple(value(n) for n in ("kBlock", "kRows", "kHistTarget", "kApplyTarget", "kClaheReplicas"))


def cell_bounds(n, side, tiles):
    """The first coordinate of cells -1 .. tiles of an axis of ``n`` frame elements (``cell_start``): cell k holds
    the coordinates whose ``floor(x / side - 0.5)``, in float32 as the pixels compute it, is k."""
    x = np.arange(n, dtype=np.int64).astype(np.float32)
    raw = np.floor(x * (R.F(1.0) / R.F(side)) - R.F(0.5)).astype(np.int64)
    assert np.all(np.diff(raw) >= 0) and raw[0] == -1 and raw[-1] <= tiles - 1
    return [int(np.searchsorted(raw, k)) for k in range(-1, tiles + 1)]


def ceil_div(a, b):
    return -(-a // b)


def passes(nbytes):
    """``(passes, lanes in the last pass)`` of ``for (b = t; b < nbytes; b += kBlock)``."""
    p = ceil_div(nbytes, K_BLOCK)
    return p, nbytes - (p - 1) * K_BLOCK


def rounds(rows):
    """The rows each ``kRows`` round of a slice of ``rows`` rows counts, e.g. 9 -> [4, 4, 1]."""
    return [min(K_ROWS, rows - r) for r in range(0, rows, K_ROWS)]


def strip_cut(cell_rows, strips):
    """``(rows of every strip that has any, strips that return at y0 >= yhi)`` of a cell of ``cell_rows`` rows."""
    per = ceil_div(cell_rows, strips)
    sizes = [min(per, cell_rows - i * per) for i in range(strips) if i * per < cell_rows]
    assert sum(sizes) == cell_rows
    return sizes, strips - len(sizes)


Plan = collections.namedtuple("Plan", "th tw rows slices last_slice hist_bytes strips cell_w cell_h")


def plan(h, w, grid, c, hist_wgs=HIST_TARGET, apply_wgs=APPLY_TARGET):
    """``launch_all``'s cut of an ``h x w`` frame of ``c`` channels.  ``rows``: the rows of a histogram slice,
    ``slices`` of them a tile, the last of ``last_slice`` rows; ``hist_bytes``: a tile row; ``strips``: the blend's
    workgroups a cell; ``cell_w``, ``cell_h``: the cells' sides in pixels, empty ones left out."""
    tiles_x, tiles_y = grid
    _, _, th, tw = R.geometry(h, w, tiles_x, tiles_y)
    slices = min(max(ceil_div(hist_wgs, tiles_x * tiles_y), 1), th, 65535)
    rows = ceil_div(th, slices)
    slices = ceil_div(th, rows)
    strips = min(max(ceil_div(apply_wgs, (tiles_x + 1) * (tiles_y + 1)), 1), th, 65535)
    xs, ys = cell_bounds(w, tw, tiles_x), cell_bounds(h, th, tiles_y)
    assert xs[0] == 0 and xs[-1] == w and ys[0] == 0 and ys[-1] == h
    return Plan(th, tw, rows, slices, th - (slices - 1) * rows, tw * c, strips,
                [b - a for a, b in zip(xs, xs[1:]) if b > a], [b - a for a, b in zip(ys, ys[1:]) if b > a])
