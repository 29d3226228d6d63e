"""The comparisons a variant child runs (``tests/_variant_child.py``) and ``tests/test_gpu_variants.py`` counts: the
histogram, the level filter, the table filter and CLAHE against the numpy references their own tests use.  The
frames are ``tests/test_gpu_grid_stride.py``'s A (317 x 331 x 3, and the same bytes as one channel of 317 x 993) and
``tests/_clahe_shapes.py``'s cases a, b and c; nothing is made here that those files make.  ``comparisons()`` only
lists: a frame or a reference is made when its comparison runs."""
import numpy as np

import _clahe_ref as CR
import _level_ref as LR
from _clahe_shapes import CASES
from test_gpu_clahe import _filter as clahe_filter
from test_gpu_clahe import _frame as clahe_frame
from test_gpu_grid_stride import TABLES, A, _Dev, _frame, _lut_ref, _nbytes

EXPECTED = 58  # len(comparisons()): a literal, so that a list that lost its cases does not agree with itself
CONTENTS = ["random", "constant", "channel_constants"]  # constant: every lane of a wave adds to one bin
RULES = [("equalize", LR.EQUALIZE, (0, 0)), ("stretch1pc", LR.STRETCH, (655, 655))]


def _hist_device(ctx, content, c, off):
    img = _frame(content, A, c)
    got = np.empty((c, 256), np.uint32)
    with _Dev(ctx, _nbytes(A), 1) as dev:
        dh = ctx.alloc_device(3 * 1024)
        try:
            ctx.hist_device(dev.put(0, off, img.reshape(-1)), img.nbytes, c, dh)
            ctx.sync()
            ctx.download(got, dh, c * 1024)
            ctx.sync()
        finally:
            ctx.free_device(dh)
    return got, LR.hist(img)


def _calc_hist(ctx, content, c):
    import vfilter
    img = _frame(content, A, c)
    return vfilter.calc_hist(img, ctx=ctx), LR.hist(img)


def _level_device(ctx, content, c, rule, clips, off):
    img = _frame(content, A, c)
    h, w = img.shape[:2]
    with _Dev(ctx, _nbytes(A)) as dev:
        got = dev.run(img.reshape(-1), off, off, lambda s, d: ctx.level_device(s, d, w, h, c, rule, 0, 0, *clips),
                      ("level", content, c, rule, off))
    return got, LR.level(img, rule, 0, 0, clips).reshape(-1)


def _lut_device(ctx, name, off):
    import vfilter
    src = _frame("random", A).reshape(-1)
    planar, channels = vfilter.as_table(TABLES[name])
    with _Dev(ctx, _nbytes(A)) as dev:
        got = dev.run(src, off, off, lambda s, d: ctx.lut_device(s, d, src.nbytes, planar, channels), ("lut", name, off))
    return got, _lut_ref(src, TABLES[name])


def _clahe(ctx, case, content, c):
    import vfilter
    h, w, grid = CASES[case]
    img = clahe_frame(content, h, w, c, grid)
    return vfilter.clahe_frames([img], clahe_filter(512, grid), ctx=ctx)[0], CR.clahe(img, 512, grid[0], grid[1])


def comparisons():
    """``[(name, run)]``: ``run(ctx)`` gives ``(got, want)``, two arrays that have to be equal."""
    out = []
    for c in (1, 3):
        for content in CONTENTS:
            for off in (0, 7):
                out.append(("hist_device %s c%d +%d" % (content, c, off),
                            lambda ctx, content=content, c=c, off=off: _hist_device(ctx, content, c, off)))
            out.append(("calc_hist %s c%d" % (content, c), lambda ctx, content=content, c=c: _calc_hist(ctx, content, c)))
            for rname, rule, clips in RULES:
                for off in (0, 7):
                    out.append(("level_device %s %s c%d +%d" % (rname, content, c, off),
                                lambda ctx, content=content, c=c, rule=rule, clips=clips, off=off:
                                _level_device(ctx, content, c, rule, clips, off)))
    for name in ("perm1", "perm3"):
        for off in (0, 7):
            out.append(("lut_device %s +%d" % (name, off), lambda ctx, name=name, off=off: _lut_device(ctx, name, off)))
    for case in ("a", "b", "c"):
        for c in (1, 3):
            for content in ("random", "channel_constants"):
                out.append(("clahe %s %s c%d" % (case, content, c),
                            lambda ctx, case=case, content=content, c=c: _clahe(ctx, case, content, c)))
    return out
