"""ChainWorker: the reference's filter plugin with a chain of filters in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for a real filter rarely writes one call: ``cv2.morphologyEx(frame, cv2.MORPH_OPEN,
element)`` on a mask, a median blur followed by a morphological gradient and a threshold, a
difference of two blurs.  ``ChainWorker`` is ``InverterWorker`` with such a program in place of the
inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Chain`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` -- one decode, the program's steps on the pixels, one encode --
              for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_chain_frames_host`` (one upload, the steps, one download) for ``__call__`` and
              ``process_batch``; batches run synchronously and the frame's shape comes from the
              batch's wire v1 / v2 metadata, else the worker's ``shape=``, as ``RankWorker``'s does.

``chain`` is a ``vfilter.filters.Chain`` (``Morph(op, element, iterations, border)`` builds those of
``cv2.morphologyEx``).  The command line covers ``Morph``; arbitrary chains are for callers of the
class.
"""
from __future__ import annotations

import argparse

from . import elements
from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import MORPH_OPS, Chain, Morph
from .inverter import worker_main


class ChainWorker(ShapedFilterWorker):
    def __init__(self, *args, chain: Chain, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(chain, Chain):  # a Chain refused a bad program when it was built
            raise ValueError("ChainWorker: chain is a vfilter.filters.Chain (Chain([...]), Morph(op, element))")
        super().__init__(*args, filter=chain, shape=shape, **kw)
        if self.verbose:
            print(f"chain worker: a program of {len(chain)} steps")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        if channels != 3 and self.filter.table_channels == 3:
            raise ValueError("the chain has a 3-channel table; raw frames have 3 channels")
        if channels != 3 and self.filter.has_mix:
            raise ValueError("the chain has a colour matrix; raw frames have 3 channels")
        self.ctx.chain_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def morph_from_options(op: str, element: str = "rect", size=(3,), iterations: int = 1, border=None) -> Chain:
    """The ``Chain`` of the command line's ``--morph``, ``--element``, ``--size W [H]``,
    ``--iterations`` and ``--border``; a bad combination raises ``ValueError``."""
    size = tuple(size)
    if len(size) not in (1, 2):
        raise ValueError(f"--size takes W or W H, not {len(size)} values")
    if op not in MORPH_OPS:
        raise ValueError(f"--morph must be one of {list(MORPH_OPS)}, not {op!r}")
    if element not in ("rect", "cross"):
        raise ValueError(f"--element must be rect or cross, not {element!r}")
    w, h = size[0], size[-1]
    e = elements.rect(w, h) if element == "rect" else elements.cross(w, h)
    return Morph(op, e, iterations, "constant" if border is None else border)


def main(argv=None):
    """The inverter worker's command line plus ``--morph``, ``--element``, ``--size``, ``--iterations``,
    ``--border`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="cv2.morphologyEx (open, close, gradient, top-hat, black-hat, ...) worker "
                                             "for video processing (MI355X backend)")
    ap.add_argument("--morph", choices=MORPH_OPS, required=True, metavar="OP", help=" | ".join(MORPH_OPS))
    ap.add_argument("--element", choices=("rect", "cross"), default="rect", help="the structuring element's form")
    ap.add_argument("--size", type=int, nargs="+", default=[3], metavar="N",
                    help="the element's sides W [H], odd and at most 7; default 3")
    ap.add_argument("--iterations", type=int, default=1,
                    help="successive erosions / dilations; limited by the chain's 8 steps")
    ap.add_argument("--border", choices=("reflect101", "replicate", "constant"), default=None,
                    help="default: constant (a tap outside the frame is left out), cv2.morphologyEx's")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        chain = morph_from_options(args.morph, args.element, args.size, args.iterations, args.border)  # a bad
        _shape3(args.shape)                                   # combination ends here, before a GPU context exists
        return {"chain": chain, "shape": args.shape}

    worker_main(ap, argv, "chain worker", ChainWorker, own)


if __name__ == "__main__":
    main()
