"""``tests/_chain_ref.py``'s interpreter extended by the level step, without editing it:

    ("level", a, rule, mask, link, (clip_lo, clip_hi))      _level_ref.level's arguments

with the colour-matrix step of ``_chain_ref_mix`` and the separable step of ``_chain_ref_sep`` as well;
every other step is handed to ``_chain_ref``.  A level step reads its whole operand, so the
interpreter's whole-frame semantics is the only one there is.  Shares no code with ``vfilter``.
"""
import numpy as np

import _chain_ref as CR
import _level_ref as L
import _mix_ref as M
import _sep_ref as S


def run(img, prog):
    """The program's result on the whole frame ``img`` (uint8 H x W or H x W x C)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and 1 <= len(prog) <= CR.MAX_STEPS
    vals = [img]
    for st in prog:
        if st[0] == "level":
            out = L.level(vals[st[1]], *st[2:])
        elif st[0] == "mix":
            out = M.mix(vals[st[1]], st[2], st[3], st[4])
        elif st[0] == "sep":
            out = S.sep(vals[st[1]], *st[2:])
        elif st[0] == "bin":
            out = CR.binary(st[1], vals[st[2]], vals[st[3]])
        else:  # a one-step program on the operand
            out = CR.run(vals[st[1]], [(st[0], 0) + tuple(st[2:])])
        assert out.shape == img.shape and out.dtype == np.uint8
        vals.append(out)
    return vals[-1]
