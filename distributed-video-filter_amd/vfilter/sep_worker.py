"""SepWorker: the reference's filter plugin with a separable filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for ``cv2.blur(frame, (5, 5))``, a ``cv2.boxFilter``, a wide Gaussian or any
``cv2.sepFilter2D`` has ``SepWorker``: ``InverterWorker`` with that call in place of the inversion
and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Separable`` as the worker's filter: the GPU pass
              of ``TurboJPEG.filter_*`` (decode -> filter -> encode, no host round trip of the
              pixels) for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_sep_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``ConvWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).

``sep`` is a ``vfilter.filters.Separable``.
"""
from __future__ import annotations

import argparse

import numpy as np

from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import BORDERS, ROUNDINGS, Separable
from .inverter import worker_main


class SepWorker(ShapedFilterWorker):
    def __init__(self, *args, sep: Separable, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(sep, Separable):  # a Separable refused bad taps or a bad scale when it was built
            raise ValueError("SepWorker: sep is a vfilter.filters.Separable")
        super().__init__(*args, filter=sep, shape=shape, **kw)
        if self.verbose:
            scale = f"/ {sep.divisor}" if sep.divisor != 1 else f"/ 2^{sep.shift}, {sep.rounding}"
            print(f"separable-filter worker: {sep.kx.size} x {sep.ky.size} taps {scale}, {sep.border}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        self.ctx.sep_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def sep_from_options(box=None, gaussian=None, kx_npy=None, ky_npy=None, shift=None, divisor=None, rounding=None,
                     border="reflect101") -> Separable:
    """The ``Separable`` of the command line's options; a bad combination raises ``ValueError``."""
    chosen = [name for name, v in (("--box", box), ("--gaussian", gaussian), ("--kx-npy", kx_npy)) if v is not None]
    if len(chosen) != 1:
        raise ValueError("give exactly one of --box, --gaussian and --kx-npy" +
                         (f", not {' and '.join(chosen)}" if chosen else ""))
    if rounding is not None and rounding not in ROUNDINGS:
        raise ValueError(f"--rounding must be one of {sorted(ROUNDINGS)}, not {rounding!r}")
    if border not in BORDERS:
        raise ValueError(f"--border must be one of {sorted(BORDERS)}, not {border!r}")
    if ky_npy is not None and kx_npy is None:
        raise ValueError("--ky-npy goes with --kx-npy")
    if box is not None:
        if shift is not None or rounding is not None:
            raise ValueError("--box divides by its area (or, with --divisor 1, sums); it takes no --shift or --rounding")
        if divisor not in (None, 1):
            raise ValueError("--box divides by its area; --divisor 1 alone is allowed, for the saturating sum")
        if len(box) not in (1, 2):
            raise ValueError("--box takes W [H]")
        return Separable.box(tuple(box) if len(box) == 2 else box[0], divisor is None, border)
    if gaussian is not None:
        if shift is not None or divisor is not None:
            raise ValueError("--gaussian carries its own scale; it takes no --shift or --divisor")
        ksize, sigma = gaussian
        if float(ksize) != int(ksize):
            raise ValueError(f"--gaussian KSIZE SIGMA: KSIZE = {ksize} is not an integer")
        return Separable.gaussian(int(ksize), float(sigma), rounding=rounding or "half_up", border=border)
    kx = np.load(kx_npy, allow_pickle=False)
    ky = None if ky_npy is None else np.load(ky_npy, allow_pickle=False)
    return Separable(kx, ky, shift, divisor, rounding or "half_even", border)


def main(argv=None):
    """The inverter worker's command line plus ``--box``, ``--gaussian``, ``--kx-npy`` / ``--ky-npy``, ``--shift``,
    ``--divisor``, ``--rounding``, ``--border`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="separable filter (cv2.sepFilter2D, cv2.blur, cv2.boxFilter, Gaussian) "
                                             "worker for video processing (MI355X backend)")
    ap.add_argument("--box", type=int, nargs="+", default=None, metavar="N", help="cv2.blur: W [H], odd, up to 31")
    ap.add_argument("--gaussian", type=float, nargs=2, default=None, metavar=("KSIZE", "SIGMA"),
                    help="a fixed-point Gaussian of KSIZE taps an axis (vfilter.kernels.gaussian_taps, 8 bits)")
    ap.add_argument("--kx-npy", default=None, metavar="PATH", help="numpy file with the horizontal taps (1-D)")
    ap.add_argument("--ky-npy", default=None, metavar="PATH", help="numpy file with the vertical taps (default: kx)")
    ap.add_argument("--shift", type=int, default=None, help="divide the sum by 2**SHIFT (0..16)")
    ap.add_argument("--divisor", type=int, default=None, help="divide the sum by the odd DIVISOR (up to 1023)")
    ap.add_argument("--rounding", choices=sorted(ROUNDINGS), default=None,
                    help="default: half_even (--gaussian: half_up)")
    ap.add_argument("--border", choices=sorted(BORDERS), default="reflect101")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W [C] (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        sep = sep_from_options(args.box, args.gaussian, args.kx_npy, args.ky_npy, args.shift, args.divisor,
                               args.rounding, args.border)  # a bad combination ends here,
        _shape3(args.shape)                                 # before a GPU context exists
        return {"sep": sep, "shape": args.shape}

    worker_main(ap, argv, "separable-filter worker", SepWorker, own)


if __name__ == "__main__":
    main()
