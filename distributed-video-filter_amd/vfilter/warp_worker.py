"""WarpWorker: the reference's filter plugin with an affine warp in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for ``cv2.flip`` or ``cv2.warpAffine`` -- mirroring a webcam, de-rotating a tilted
camera, a digital zoom or a sub-pixel shift for stabilisation -- has ``WarpWorker``:
``InverterWorker`` with that call in place of the inversion and the same plugin contract,
``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Warp`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> warp -> encode, no host round trip of the pixels)
              for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_warp_frames_host`` (upload, one kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  A frame that
              does not fit the context's staging whole is refused.

``warp`` is a ``vfilter.filters.Warp``.  Frames keep their size.
"""
from __future__ import annotations

import argparse

from . import warps
from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import Warp
from .inverter import worker_main


class WarpWorker(ShapedFilterWorker):
    def __init__(self, *args, warp: Warp, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(warp, Warp):  # a Warp refused a bad matrix, flip or border when it was built
            raise ValueError("WarpWorker: warp is a vfilter.filters.Warp")
        super().__init__(*args, filter=warp, shape=shape, **kw)
        if self.verbose:
            what = f"flip mode {warp.mode}" if warp.mode else f"map (destination to source) {warp.m}"
            print(f"warp worker: {what}, {warp.interpolation}, border {warp.border} {warp.value}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.warp_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def main(argv=None):
    """The inverter worker's command line plus one of ``--flip``, ``--rotate`` (with ``--scale`` and ``--center``) and
    ``--matrix``, and ``--interpolation``, ``--border``, ``--border-value`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="affine warp (cv2.warpAffine, cv2.flip) worker for video processing (MI355X backend)")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--flip", choices=["h", "v", "both"], help="mirror every frame, whatever its size")
    what.add_argument("--rotate", type=float, metavar="DEG", help="rotate by DEG degrees counter-clockwise about --center")
    what.add_argument("--matrix", type=float, nargs=6, metavar=("a", "b", "c", "d", "e", "f"),
                      help="the forward 2 x 3 map [[a b c] [d e f]], as cv2.warpAffine takes it")
    ap.add_argument("--scale", type=float, default=1.0, metavar="S", help="with --rotate: the scale (default: 1)")
    ap.add_argument("--center", type=float, nargs=2, default=None, metavar=("X", "Y"),
                    help="with --rotate: the fixed point (default: the centre of --shape)")
    ap.add_argument("--interpolation", choices=["linear", "nearest"], default="linear")
    ap.add_argument("--border", choices=["constant", "replicate", "reflect101"], default="constant")
    ap.add_argument("--border-value", type=int, nargs="+", default=[0], metavar="V", help="the constant border: V or B G R")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        h, w, _ = _shape3(args.shape)
        value = args.border_value[0] if len(args.border_value) == 1 else args.border_value
        if args.flip:  # a bad value ends here, before a GPU context
            warp = Warp(flip=args.flip, interpolation="nearest", border=args.border, border_value=value)
        else:
            if args.matrix is not None:
                m = [args.matrix[:3], args.matrix[3:]]
            else:
                m = warps.rotation(args.center or ((w - 1) / 2, (h - 1) / 2), args.rotate, args.scale)
            warp = Warp(m, None, args.interpolation, args.border, value)
        return {"warp": warp, "shape": args.shape}

    worker_main(ap, argv, "warp worker", WarpWorker, own)


if __name__ == "__main__":
    main()
