"""A reference program of ``tests/_chain_ref.py`` as the ``vfilter.Chain`` that should compute it."""
import numpy as np

from vfilter.filters import Chain, Kernel, Rank, Table


def to_chain(prog) -> Chain:
    entries = []
    for st in prog:
        if st[0] == "table":
            entries.append((Table(np.asarray(st[2])), st[1]))
        elif st[0] == "conv":
            entries.append((Kernel((np.asarray(st[2]), st[3]), st[4]), st[1]))
        elif st[0] == "rank":
            f = Rank.median(st[3]) if st[2] == "median" else Rank(st[2], st[3], st[4])
            entries.append((f, st[1]))
        else:
            entries.append((st[1], st[2], st[3]))
    return Chain.program(entries)
