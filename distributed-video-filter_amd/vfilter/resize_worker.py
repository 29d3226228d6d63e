"""ResizeWorker: the reference's filter plugin with a resize in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for ``cv2.resize`` -- 4K down to 1080p, a thumbnail, a 2 x upscale for display -- has
``ResizeWorker``: ``InverterWorker`` with that call in place of the inversion and the same plugin
contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Resize`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> resize -> encode, no host round trip of the pixels)
              for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.  A
              result is a JPEG of its own size, as every JPEG result is.
  raw mode    ``vf_resize_frames_host`` (upload, one kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  The result has
              another length than the frame: ``process_raw_batch`` allocates every result at its own
              size (a caller's ``outs`` entry is used only where it has exactly that length), and
              through ``worker.py`` it travels with ``nbytes`` set and ``shape=None``.  A result
              shape in the reply is out of scope: the receiver computes it with
              ``Resize.out_size``.

``resize`` is a ``vfilter.filters.Resize``.
"""
from __future__ import annotations

import argparse
import time

import numpy as np

from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import Resize
from .inverter import worker_main


class ResizeWorker(ShapedFilterWorker):
    def __init__(self, *args, resize: Resize, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(resize, Resize):  # a Resize refused a bad size, scale or interpolation when it was built
            raise ValueError("ResizeWorker: resize is a vfilter.filters.Resize")
        super().__init__(*args, filter=resize, shape=shape, **kw)
        if self.verbose:
            what = f"to {resize.dsize}" if resize.dsize else f"by fx={resize.fx}, fy={resize.fy}"
            print(f"resize worker: {what}, {resize.interpolation}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.resize_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)

    def _result_bytes(self, nbytes: int, meta=None) -> int:
        h, w, c = self._frame_shape(nbytes, meta)
        ow, oh = self.filter.out_size(w, h)
        return ow * oh * c

    def unfused_call(self, frame_bytes):
        if self.delay > 0:                                          # inverter.py:37-38
            time.sleep(self.delay)
        frame = np.frombuffer(frame_bytes, dtype=np.uint8)          # inverter.py:34
        out = np.empty(self._result_bytes(frame.nbytes), np.uint8)
        self.raw_batch([frame], [None], [out])
        return out

    def process_raw_batch(self, frames, metas, outs, srcs, dsts) -> list:
        """Every result at its own size: ``dsts`` were made at the frames' sizes and are not used."""
        try:
            sized = []
            for s, m, o in zip(srcs, metas, outs):
                n = self._result_bytes(s.nbytes, m)
                sized.append(o if isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.ndim == 1 and o.nbytes == n
                             and o.flags.c_contiguous else np.empty(n, np.uint8))
            self.raw_batch(srcs, metas, sized)
        except Exception as e:  # frame by frame, so that a bad frame fails alone
            results = []
            for s, m in zip(srcs, metas):
                try:
                    out = np.empty(self._result_bytes(s.nbytes, m), np.uint8)
                    self.raw_batch([s], [m], [out])
                    results.append(out)
                except Exception as one:
                    results.append(one)
            return results if results else [e] * len(frames)
        return sized


def main(argv=None):
    """The inverter worker's command line plus ``--dsize W H`` or ``--fx F --fy F``, ``--interpolation`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="resize (cv2.resize) worker for video processing (MI355X backend)")
    ap.add_argument("--dsize", type=int, nargs=2, default=None, metavar=("W", "H"), help="the result's size")
    ap.add_argument("--fx", type=float, default=0.0, metavar="F", help="without --dsize: the horizontal scale")
    ap.add_argument("--fy", type=float, default=0.0, metavar="F", help="without --dsize: the vertical scale")
    ap.add_argument("--interpolation", choices=["nearest", "linear", "area"], default="linear")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        _shape3(args.shape)
        # a bad value ends here, before a GPU context
        return {"resize": Resize(tuple(args.dsize) if args.dsize else None, args.fx, args.fy, args.interpolation),
                "shape": args.shape}

    worker_main(ap, argv, "resize worker", ResizeWorker, own)


if __name__ == "__main__":
    main()
