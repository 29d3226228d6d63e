"""``tests/_chain_ref_level.py``'s interpreter extended by the CLAHE step, without editing it:

    ("clahe", a, clip_q8, tiles_x, tiles_y, mask)      _clahe_ref.clahe's arguments

every other step is handed on.  A CLAHE step reads its whole operand, so the interpreter's
whole-frame semantics is the only one there is.  Shares no code with ``vfilter``.
"""
import numpy as np

import _chain_ref as CR
import _chain_ref_level as CL
import _clahe_ref as C


def run(img, prog):
    """The program's result on the whole frame ``img`` (uint8 H x W or H x W x C)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and 1 <= len(prog) <= CR.MAX_STEPS
    vals = [img]
    for st in prog:
        if st[0] == "clahe":
            out = C.clahe(vals[st[1]], *st[2:])
        elif st[0] == "bin":
            out = CR.binary(st[1], vals[st[2]], vals[st[3]])
        else:  # a one-step program on the operand
            out = CL.run(vals[st[1]], [(st[0], 0) + tuple(st[2:])])
        assert out.shape == img.shape and out.dtype == np.uint8
        vals.append(out)
    return vals[-1]
