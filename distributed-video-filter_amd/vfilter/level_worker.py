"""LevelWorker: the reference's filter plugin with histogram equalisation or auto-levels in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for ``cv2.equalizeHist``, an auto-contrast or a min-max normalisation -- a table that
is computed from the frame itself -- has ``LevelWorker``: ``InverterWorker`` with that call in place
of the inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Level`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> histogram -> table -> encode, no host round trip of
              the pixels or of the histogram) for ``__call__``, ``process_batch``, ``submit_batch``
              and ``submit_ring_batch``.
  raw mode    ``vf_level_frames_host`` (upload, the two kernels, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  A frame that
              does not fit the context's staging whole is refused.

``level`` is a ``vfilter.filters.Level``.
"""
from __future__ import annotations

import argparse

from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import Level
from .inverter import worker_main


class LevelWorker(ShapedFilterWorker):
    def __init__(self, *args, level: Level, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(level, Level):  # a Level refused a bad rule, clip or channel when it was built
            raise ValueError("LevelWorker: level is a vfilter.filters.Level")
        super().__init__(*args, filter=level, shape=shape, **kw)
        if self.verbose:
            what = "equalize" if level.rule == "equalize" else f"stretch, clips {level.clip_lo} and {level.clip_hi} / 65536"
            chans = "all channels" if level.mask == 0 else f"channel mask {level.mask}"
            print(f"level worker: {what}, {chans}{', linked' if level.link else ''}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.level_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def level_from_options(equalize: bool = False, stretch=None, channels=None, link: bool = False) -> Level:
    """The ``Level`` of the command line's options; a bad combination raises ``ValueError``."""
    if equalize == (stretch is not None):
        raise ValueError("give exactly one of --equalize and --stretch" + (", not both" if equalize else ""))
    if equalize:
        return Level.equalize(channels, link)
    if len(stretch) not in (1, 2):
        raise ValueError("--stretch takes CLIP, or CLIP_LO CLIP_HI")
    return Level.stretch(stretch[0] if len(stretch) == 1 else tuple(stretch), channels, link)


def main(argv=None):
    """The inverter worker's command line plus ``--equalize`` | ``--stretch CLIP``, ``--channels``, ``--link`` and
    ``--shape``."""
    ap = argparse.ArgumentParser(description="histogram equalisation / auto-levels (cv2.equalizeHist) worker for video "
                                             "processing (MI355X backend)")
    ap.add_argument("--equalize", action="store_true", help="cv2.equalizeHist on every levelled channel")
    ap.add_argument("--stretch", type=float, nargs="+", default=None, metavar="CLIP",
                    help="auto-levels: CLIP (or CLIP_LO CLIP_HI), the fraction of pixels clipped at each end, in [0, 0.5)")
    ap.add_argument("--channels", type=int, nargs="+", default=None, metavar="C",
                    help="the channels that are levelled, among 0 1 2 (default: all)")
    ap.add_argument("--link", action="store_true", help="one table for the levelled channels, from their summed histograms")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        level = level_from_options(args.equalize, args.stretch, args.channels, args.link)  # a bad combination ends
        _shape3(args.shape)                                                                # here, before a GPU context
        return {"level": level, "shape": args.shape}

    worker_main(ap, argv, "level worker", LevelWorker, own)


if __name__ == "__main__":
    main()
