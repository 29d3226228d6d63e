"""RankWorker: the reference's filter plugin with a rank filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for a despeckle or a mask clean-up writes ``cv2.medianBlur(frame, ksize)``,
``cv2.erode(frame, element)`` or ``cv2.dilate(frame, element)``.  ``RankWorker`` is
``InverterWorker`` with that call in place of the inversion and the same plugin contract,
``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Rank`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> filter -> encode, no host round trip of the pixels)
              for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_rank_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  A frame of
              another size fails alone, as the reference's reshape does (worker.py:74-76).

``rank`` is a ``vfilter.filters.Rank`` (``Rank.erode(element, border)``, ``Rank.dilate(...)``,
``Rank.median(ksize)``); the filter is applied to each channel.
"""
from __future__ import annotations

import argparse

from . import elements
from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import Rank
from .inverter import worker_main


class RankWorker(ShapedFilterWorker):
    def __init__(self, *args, rank: Rank, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(rank, Rank):  # a Rank refused a bad element or border when it was built
            raise ValueError("RankWorker: rank is a vfilter.filters.Rank (Rank.erode, Rank.dilate, Rank.median)")
        super().__init__(*args, filter=rank, shape=shape, **kw)
        if self.verbose:
            kh, kw_ = rank.element.shape
            print(f"rank worker: {rank.op}, {kh} x {kw_} element, {rank.border}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.rank_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def rank_from_options(op: str, element: str = "rect", size=(3,), border=None) -> Rank:
    """The ``Rank`` of the command line's ``--op``, ``--element``, ``--size W [H]`` and ``--border``;
    a bad combination raises ``ValueError``."""
    size = tuple(size)
    if len(size) not in (1, 2):
        raise ValueError(f"--size takes W or W H, not {len(size)} values")
    w, h = size[0], size[-1]
    if op == "median":
        if element != "rect" or w != h:
            raise ValueError("--op median takes the full square: --element rect and one --size")
        if border not in (None, "replicate"):
            raise ValueError("--op median replicates the border (cv2.medianBlur has no other)")
        return Rank.median(w)
    if op not in ("erode", "dilate"):
        raise ValueError(f"--op must be erode, dilate or median, not {op!r}")
    if element not in ("rect", "cross"):
        raise ValueError(f"--element must be rect or cross, not {element!r}")
    e = elements.rect(w, h) if element == "rect" else elements.cross(w, h)
    return Rank(op, e, "constant" if border is None else border)


def main(argv=None):
    """The inverter worker's command line plus ``--op``, ``--element``, ``--size``, ``--border`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="erode / dilate / median (cv2.erode, cv2.dilate, cv2.medianBlur) worker "
                                             "for video processing (MI355X backend)")
    ap.add_argument("--op", choices=("erode", "dilate", "median"), required=True)
    ap.add_argument("--element", choices=("rect", "cross"), default="rect",
                    help="the structuring element's form (median: rect, the full square)")
    ap.add_argument("--size", type=int, nargs="+", default=[3], metavar="N",
                    help="the element's sides W [H], odd and at most 7 (median: 3 or 5); default 3")
    ap.add_argument("--border", choices=("reflect101", "replicate", "constant"), default=None,
                    help="default: constant for erode and dilate (a tap outside the frame is left out), "
                         "replicate for median (the only one)")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        rank = rank_from_options(args.op, args.element, args.size, args.border)  # a bad combination ends here,
        _shape3(args.shape)                                                     # before a GPU context exists
        return {"rank": rank, "shape": args.shape}

    worker_main(ap, argv, "rank worker", RankWorker, own)


if __name__ == "__main__":
    main()
