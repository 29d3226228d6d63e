"""ClaheWorker: the reference's filter plugin with CLAHE in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for ``cv2.createCLAHE(clip, grid).apply`` -- the contrast filter people put on video,
which does not blow out a frame with a bright window in it as global equalisation does -- has
``ClaheWorker``: ``InverterWorker`` with that call in place of the inversion and the same plugin
contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Clahe`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> tile histograms -> tables -> blend -> encode, no host
              round trip of the pixels or of the tables) for ``__call__``, ``process_batch``,
              ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_clahe_frames_host`` (upload, the three kernels, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  A frame that
              does not fit the context's staging whole is refused.

``clahe`` is a ``vfilter.filters.Clahe``.
"""
from __future__ import annotations

import argparse

from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import Clahe
from .inverter import worker_main


class ClaheWorker(ShapedFilterWorker):
    def __init__(self, *args, clahe: Clahe, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(clahe, Clahe):  # a Clahe refused a bad limit, grid or channel when it was built
            raise ValueError("ClaheWorker: clahe is a vfilter.filters.Clahe")
        super().__init__(*args, filter=clahe, shape=shape, **kw)
        if self.verbose:
            chans = "all channels" if clahe.mask == 0 else f"channel mask {clahe.mask}"
            print(f"clahe worker: clip limit {clahe.clip_limit}, {clahe.tiles_x} x {clahe.tiles_y} tiles, {chans}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.clahe_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def main(argv=None):
    """The inverter worker's command line plus ``--clip-limit``, ``--tiles``, ``--channels`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="CLAHE (cv2.createCLAHE) worker for video processing (MI355X backend)")
    ap.add_argument("--clip-limit", type=float, default=40.0, metavar="LIMIT",
                    help="the clip limit; LIMIT * 256 must be an integer, 0: no clipping (default: 40.0, cv2's)")
    ap.add_argument("--tiles", type=int, nargs=2, default=[8, 8], metavar=("X", "Y"),
                    help="the tile grid, 1 .. 16 an axis (default: 8 8, cv2's)")
    ap.add_argument("--channels", type=int, nargs="+", default=None, metavar="C",
                    help="the channels that are filtered, among 0 1 2 (default: all)")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        clahe = Clahe(args.clip_limit, tuple(args.tiles), args.channels)  # a bad value ends here, before a GPU context
        _shape3(args.shape)
        return {"clahe": clahe, "shape": args.shape}

    worker_main(ap, argv, "clahe worker", ClaheWorker, own)


if __name__ == "__main__":
    main()
