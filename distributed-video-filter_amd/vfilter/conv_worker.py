"""ConvWorker: the reference's filter plugin with a neighbourhood filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for a blur, a Gaussian, a sharpening or an edge filter has one call,
``cv2.filter2D(frame, -1, kernel)``.  ``ConvWorker`` is ``InverterWorker`` with that call in place
of the inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Kernel`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> filter2D -> encode, no host round trip of the
              pixels) for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_conv_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``LutWorker``'s do.  Unlike a
              per-pixel filter this one needs the frame's shape: a batch's wire v1 / v2 metadata
              carries it; without it (wire v0, ``__call__``) the worker's ``shape=`` applies,
              by default the reference's 480 x 480 x 3 (inverter.py:34).  A frame of another
              size fails alone, as the reference's reshape does (worker.py:74-76).

``kernel`` and ``border`` are as for ``vfilter.filter2d``; the kernel is applied to each channel.
"""
from __future__ import annotations

import argparse

import numpy as np

from .filters import Kernel
from .inverter import FilterWorker, worker_main

DEFAULT_SHAPE = (480, 480, 3)  # inverter.py:34


def _shape3(shape) -> tuple:
    s = tuple(int(v) for v in shape)
    if len(s) == 2:
        s = s + (1,)
    if len(s) != 3 or s[2] not in (1, 3) or s[0] <= 0 or s[1] <= 0:
        raise ValueError(f"a raw frame is H x W or H x W x 3, not shape {tuple(shape)}")
    return s


class ShapedFilterWorker(FilterWorker):
    """A FilterWorker whose raw filter needs each frame's shape (ConvWorker, RankWorker): from the
    batch's wire metadata, else from ``shape=``.  A subclass adds ``frames_host``."""

    def __init__(self, *args, filter, shape=DEFAULT_SHAPE, **kw):
        self.shape = _shape3(shape)
        super().__init__(*args, filter=filter, **kw)

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        """The worker's filter on raw frames of the given sizes and one channel count."""
        raise NotImplementedError

    def _frame_shape(self, nbytes: int, meta=None) -> tuple:
        shape = _shape3(meta.shape) if meta is not None and getattr(meta, "shape", None) else self.shape
        if shape[0] * shape[1] * shape[2] != nbytes:
            raise ValueError(f"cannot reshape a raw frame of {nbytes} bytes into shape {shape}")  # inverter.py:34
        return shape

    def raw_batch(self, srcs, metas, dsts) -> None:
        shapes = [self._frame_shape(s.nbytes, m) for s, m in zip(srcs, metas)]
        chans = {s[2] for s in shapes}
        if len(chans) != 1:
            raise ValueError("the frames of one batch have one channel count")
        self.frames_host(srcs, dsts, [s[1] for s in shapes], [s[0] for s in shapes], chans.pop())


class ConvWorker(ShapedFilterWorker):
    def __init__(self, *args, kernel, border: str = "reflect101", shape=DEFAULT_SHAPE, **kw):
        filt = Kernel(kernel, border)  # refuses a bad kernel or border before any GPU work
        super().__init__(*args, filter=filt, shape=shape, **kw)
        if self.verbose:
            kh, kw = filt.weights.shape
            print(f"filter2D worker: {kh} x {kw} kernel / 2^{filt.shift}, {border}")

    @property
    def kernel(self):
        return self.filter.weights, self.filter.shift

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.conv_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def main(argv=None):
    """The inverter worker's command line plus ``--kernel-npy``, ``--shift``, ``--border`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="2-D convolution (cv2.filter2D) worker for video processing (MI355X backend)")
    ap.add_argument("--kernel-npy", required=True, metavar="PATH",
                    help="numpy file with the kernel: integer weights (see --shift) or a dyadic float kernel; "
                         "odd sides up to 7")
    ap.add_argument("--shift", type=int, default=None,
                    help="divide the integer weights' sum by 2**SHIFT (0..16), rounding half to even")
    ap.add_argument("--border", choices=("reflect101", "replicate", "constant"), default="reflect101")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        kernel = np.load(args.kernel_npy, allow_pickle=False)
        if args.shift is not None:
            kernel = (kernel, args.shift)
        Kernel(kernel, args.border)  # a bad kernel ends here, before a GPU context exists
        _shape3(args.shape)
        return {"kernel": kernel, "border": args.border, "shape": args.shape}

    worker_main(ap, argv, "filter2D worker", ConvWorker, own)


if __name__ == "__main__":
    main()
