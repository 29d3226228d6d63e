"""MixWorker: the reference's filter plugin with a colour matrix in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for a grayscale, a BGR -> RGB swap, a sepia tone, a saturation or a white balance
writes one call, ``cv2.transform(frame, m)`` (or ``cv2.cvtColor``).  ``MixWorker`` is
``InverterWorker`` with that call in place of the inversion and the same plugin contract,
``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Mix`` as the worker's filter: the GPU pass of
              ``TurboJPEG.filter_*`` (decode -> matrix -> encode, no host round trip of the pixels)
              for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_mix_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches run synchronously, as ``RankWorker``'s do, and the frame's
              shape comes from the same places: a batch's wire v1 / v2 metadata, else the worker's
              ``shape=``, by default the reference's 480 x 480 x 3 (inverter.py:34).  Frames have 3
              channels: the matrix mixes them.

``mix`` is a ``vfilter.filters.Mix`` (``vfilter.colors`` builds the usual matrices).
"""
from __future__ import annotations

import argparse

from . import colors
from .conv_worker import DEFAULT_SHAPE, ShapedFilterWorker, _shape3
from .filters import ROUNDINGS, Mix
from .inverter import worker_main

# preset -> how many numbers --params takes
PRESETS = {"identity": 0, "swap_rb": 0, "gray": 0, "sepia": 0, "saturation": 1, "gain": 3, "offset": 3,
           "gray_weights": 4}


def _mix_shape(shape) -> tuple:
    s = _shape3(shape)
    if s[2] != 3:
        raise ValueError(f"a colour matrix mixes the 3 channels of a pixel; --shape is H W 3, not {tuple(shape)}")
    return s


class MixWorker(ShapedFilterWorker):
    def __init__(self, *args, mix: Mix, shape=DEFAULT_SHAPE, **kw):
        if not isinstance(mix, Mix):  # a Mix refused a bad matrix or rounding when it was built
            raise ValueError("MixWorker: mix is a vfilter.filters.Mix (see vfilter.colors)")
        super().__init__(*args, filter=mix, shape=_mix_shape(shape), **kw)
        if self.verbose:
            print(f"colour-matrix worker: {mix.matrix.tolist()} / 2^{mix.shift}, {mix.rounding}")

    def frames_host(self, srcs, dsts, widths, heights, channels: int) -> None:
        if channels != 3:
            raise ValueError("a colour matrix on 1-channel frames; raw frames have 3 channels")
        self.ctx.mix_frames_host(srcs, dsts, widths, heights, channels, *self.filter.args)


def mix_from_options(preset: str, params=(), rounding=None) -> Mix:
    """The ``Mix`` of the command line's ``--preset``, ``--params`` and ``--rounding``; a bad
    combination raises ``ValueError``."""
    if preset not in PRESETS:
        raise ValueError(f"--preset must be one of {sorted(PRESETS)}, not {preset!r}")
    params = tuple(params or ())
    if len(params) != PRESETS[preset]:
        raise ValueError(f"--preset {preset} takes {PRESETS[preset]} --params, not {len(params)}")
    if rounding is not None and rounding not in ROUNDINGS:
        raise ValueError(f"--rounding must be one of {sorted(ROUNDINGS)}, not {rounding!r}")
    if preset in ("offset", "gray_weights"):
        if any(float(p) != int(p) for p in params):
            raise ValueError(f"--preset {preset} takes integers")
        params = tuple(int(p) for p in params)
    m = getattr(colors, preset)(*params)
    if isinstance(m, Mix):  # the preset carries its rounding (gray: half_up)
        if rounding not in (None, m.rounding):
            raise ValueError(f"--preset {preset} rounds {m.rounding}; use gray_weights for another rounding")
        return m
    return Mix(m, rounding or "half_even")


def main(argv=None):
    """The inverter worker's command line plus ``--preset``, ``--params``, ``--rounding`` and ``--shape``."""
    ap = argparse.ArgumentParser(description="colour matrix (cv2.transform: gray, BGR <-> RGB, sepia, saturation, "
                                             "white balance) worker for video processing (MI355X backend)")
    ap.add_argument("--preset", choices=sorted(PRESETS), required=True)
    ap.add_argument("--params", type=float, nargs="*", default=[], metavar="X",
                    help="saturation: S; gain: B G R (dyadic); offset: B G R (integers); gray_weights: B G R SHIFT")
    ap.add_argument("--rounding", choices=sorted(ROUNDINGS), default=None,
                    help="default: half_even (gray: half_up, as cv2.cvtColor)")
    ap.add_argument("--shape", type=int, nargs="+", default=list(DEFAULT_SHAPE), metavar="N",
                    help="raw frames without shape metadata: H W 3 (default: 480 480 3, inverter.py:34)")

    def own(args) -> dict:
        mix = mix_from_options(args.preset, args.params, args.rounding)  # a bad combination ends here,
        _mix_shape(args.shape)                                          # before a GPU context exists
        return {"mix": mix, "shape": args.shape}

    worker_main(ap, argv, "colour-matrix worker", MixWorker, own)


if __name__ == "__main__":
    main()
