"""``TurboJPEG`` on the MI355X: the JPEG half of the reference's default mode.

With ``use_jpeg=True`` (the default, inverter.py:10) the reference worker runs

    frame = self.jpeg.decode(frame_bytes)      # inverter.py:32
    inverted = cv2.bitwise_not(frame)          # inverter.py:41
    return self.jpeg.encode(inverted)          # inverter.py:44

with ``self.jpeg = TurboJPEG()`` from PyTurboJPEG (inverter.py:7,13; the app does the same at
webcam_app.py:9,24,110,140).  ``vfilter.jpeg.TurboJPEG`` keeps that class's method names,
arguments, defaults (quality 85, TJSAMP_422, TJPF_BGR) and return types, and runs them on
hand-written gfx950 kernels whose integer arithmetic is libjpeg-turbo's, so the bytes and
pixels are the ones libjpeg-turbo produces.  ``invert`` fuses the three reference lines on
the GPU (no host round trip of the pixels); ``*_batch`` forms take a list of frames and use one
batched GPU pass.

Which forward DCT libturbojpeg uses at quality < 96 depends on its version: 3.x uses the
accurate one unless ``TJFLAG_FASTDCT``; 2.x uses the fast one unless ``TJFLAG_ACCURATEDCT``.
The default here is 3.x behaviour; ``TurboJPEG(tj_version=2)`` reproduces 2.x.

No CPU fallback: without libvfilter_hip.so or a gfx950 device every call raises.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from ._lib import Context, get_context, jpeg_header
from .filters import Clahe, Invert, Kernel, Level, Morph, Rank, Resize, Separable, Table, Warp, _as_chain, _as_mix, _warp_flags

# TurboJPEG constants (turbojpeg.h / PyTurboJPEG)
TJPF_RGB, TJPF_BGR = 0, 1
TJSAMP_444, TJSAMP_422, TJSAMP_420, TJSAMP_GRAY, TJSAMP_440 = 0, 1, 2, 3, 4
TJCS_RGB, TJCS_YCbCr, TJCS_GRAY = 0, 1, 2
TJFLAG_BOTTOMUP = 2
TJFLAG_FASTUPSAMPLE = 256
TJFLAG_FASTDCT = 2048
TJFLAG_ACCURATEDCT = 4096

_SUPPORTED_FLAGS = TJFLAG_FASTUPSAMPLE | TJFLAG_FASTDCT | TJFLAG_ACCURATEDCT


class TurboJPEG:
    """Drop-in for PyTurboJPEG's ``TurboJPEG`` (inverter.py:13, webcam_app.py:24)."""

    def __init__(self, lib_path: Optional[str] = None, ctx: Optional[Context] = None, tj_version: int = 3):
        # lib_path is PyTurboJPEG's path to libturbojpeg; there is nothing to load here
        self._ctx = ctx
        self.tj_version = int(tj_version)

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = get_context()
        return self._ctx

    def _enc_flags(self, flags: int, quality: int) -> int:
        if flags & ~_SUPPORTED_FLAGS:
            raise NotImplementedError(f"TurboJPEG flags {flags:#x} not supported on the GPU path")
        fast = bool(flags & TJFLAG_FASTDCT) if self.tj_version >= 3 else \
            not (flags & TJFLAG_ACCURATEDCT) and quality < 96
        return (flags & TJFLAG_FASTUPSAMPLE) | (TJFLAG_FASTDCT if fast else 0)

    @staticmethod
    def _dec_flags(flags: int) -> int:
        if flags & ~_SUPPORTED_FLAGS:
            raise NotImplementedError(f"TurboJPEG flags {flags:#x} not supported on the GPU path")
        return flags & TJFLAG_FASTUPSAMPLE

    # -- PyTurboJPEG API -------------------------------------------------------------------
    def decode_header(self, jpeg_buf):
        """(width, height, jpeg_subsample, jpeg_colorspace)."""
        return jpeg_header(jpeg_buf)

    def decode(self, jpeg_buf, pixel_format: int = TJPF_BGR, scaling_factor=None, flags: int = 0) -> np.ndarray:
        """inverter.py:32 / webcam_app.py:140: JPEG bytes -> H x W x 3 uint8."""
        if scaling_factor not in (None, (1, 1)):
            raise NotImplementedError("scaling_factor is not supported on the GPU path")
        return self.ctx.jpeg_decode([jpeg_buf], pixel_format, self._dec_flags(flags))[0]

    def encode(self, img_array: np.ndarray, quality: int = 85, pixel_format: int = TJPF_BGR,
               jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """inverter.py:44 / webcam_app.py:110: H x W x 3 uint8 -> JPEG bytes."""
        return self.ctx.jpeg_encode([img_array], pixel_format, quality, jpeg_subsample,
                                    self._enc_flags(flags, quality))[0]

    # -- batched / fused extensions --------------------------------------------------------
    def decode_batch(self, jpeg_bufs: Sequence, pixel_format: int = TJPF_BGR, flags: int = 0) -> List[np.ndarray]:
        return self.ctx.jpeg_decode(list(jpeg_bufs), pixel_format, self._dec_flags(flags))

    def encode_batch(self, imgs: Sequence[np.ndarray], quality: int = 85, pixel_format: int = TJPF_BGR,
                     jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.ctx.jpeg_encode(list(imgs), pixel_format, quality, jpeg_subsample,
                                    self._enc_flags(flags, quality))

    # One filter value (``vfilter.filters``: Invert, Table, Kernel, Rank, Mix, Separable, Level, Clahe, Warp, Chain) between decode and encode.  The
    # ``invert*``, ``lut*`` and ``filter2d*`` methods below are these three with their filter built
    # from the call's own arguments.
    def filter_batch(self, jpeg_bufs: Sequence, filt, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                     flags: int = 0) -> List[bytes]:
        """One GPU pass over the batch (safe to call from several threads at once: each call leases
        its own codec)."""
        run = getattr(self.ctx, "jpeg_" + filt.family)
        return run(list(jpeg_bufs), *filt.args, quality, jpeg_subsample, self._enc_flags(flags, quality))

    def filter_batch_submit(self, jpeg_bufs: Sequence, filt, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                            flags: int = 0) -> int:
        """filter_batch, asynchronously: stage and queue the batch, return a ticket at once, to be
        collected with the ``invert_batch_result*`` methods.  One host thread can keep several
        batches in flight (each holds its own codec)."""
        run = getattr(self.ctx, f"jpeg_{filt.family}_submit")
        return run(list(jpeg_bufs), *filt.args, quality, jpeg_subsample, self._enc_flags(flags, quality))

    def filter_batch_submit_addrs(self, addrs, sizes, filt, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                                  flags: int = 0) -> int:
        """``filter_batch_submit`` for JPEGs given by address and size arrays (a worker's ring
        slots; the memory stays valid until the result is collected)."""
        run = getattr(self.ctx, f"jpeg_{filt.family}_submit_addrs")
        return run(addrs, sizes, *filt.args, quality, jpeg_subsample, self._enc_flags(flags, quality))

    def invert(self, jpeg_buf, quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(bitwise_not(decode(jpeg_buf)))`` (inverter.py:32 -> :41 -> :44) fused on the GPU."""
        return self.filter_batch([jpeg_buf], Invert(), quality, jpeg_subsample, flags)[0]

    def invert_batch(self, jpeg_bufs: Sequence, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                     flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Invert(), quality, jpeg_subsample, flags)

    def invert_batch_submit(self, jpeg_bufs: Sequence, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                            flags: int = 0) -> int:
        return self.filter_batch_submit(jpeg_bufs, Invert(), quality, jpeg_subsample, flags)

    def invert_batch_submit_addrs(self, addrs, sizes, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                                  flags: int = 0) -> int:
        return self.filter_batch_submit_addrs(addrs, sizes, Invert(), quality, jpeg_subsample, flags)

    # -- any other per-pixel filter: a 256-entry table (cv2.LUT) between decode and encode ----------
    def lut(self, jpeg_buf, table, quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.LUT(decode(jpeg_buf), table))`` fused on the GPU.  ``table`` as for
        ``vfilter.lut``; a 3-channel table's channel c is channel c of the decoded BGR frame."""
        return self.filter_batch([jpeg_buf], Table(table), quality, jpeg_subsample, flags)[0]

    def lut_batch(self, jpeg_bufs: Sequence, table, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                  flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Table(table), quality, jpeg_subsample, flags)

    def lut_batch_submit(self, jpeg_bufs: Sequence, table, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                         flags: int = 0) -> int:
        """The table is copied: the caller may change it at once."""
        return self.filter_batch_submit(jpeg_bufs, Table(table), quality, jpeg_subsample, flags)

    def lut_batch_submit_addrs(self, addrs, sizes, table, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                               flags: int = 0) -> int:
        return self.filter_batch_submit_addrs(addrs, sizes, Table(table), quality, jpeg_subsample, flags)

    # -- a neighbourhood filter: cv2.filter2D between decode and encode --------------------------------
    def filter2d(self, jpeg_buf, kernel, border: str = "reflect101", quality: int = 85,
                 jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.filter2D(decode(jpeg_buf), -1, kernel))`` on the GPU, the pixels never leaving
        it.  ``kernel`` and ``border`` as for ``vfilter.filter2d``; the kernel is applied to each
        channel of the decoded BGR frame."""
        return self.filter_batch([jpeg_buf], Kernel(kernel, border), quality, jpeg_subsample, flags)[0]

    def filter2d_batch(self, jpeg_bufs: Sequence, kernel, border: str = "reflect101", quality: int = 85,
                       jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Kernel(kernel, border), quality, jpeg_subsample, flags)

    def filter2d_batch_submit(self, jpeg_bufs: Sequence, kernel, border: str = "reflect101", quality: int = 85,
                              jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> int:
        """The kernel is copied: the caller may change it at once."""
        return self.filter_batch_submit(jpeg_bufs, Kernel(kernel, border), quality, jpeg_subsample, flags)

    def filter2d_batch_submit_addrs(self, addrs, sizes, kernel, border: str = "reflect101", quality: int = 85,
                                    jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> int:
        return self.filter_batch_submit_addrs(addrs, sizes, Kernel(kernel, border), quality, jpeg_subsample, flags)

    # -- rank filters: cv2.erode / cv2.dilate / cv2.medianBlur between decode and encode ---------------
    # The submit forms go through ``filter_batch_submit*`` with a ``vfilter.filters.Rank``.
    def erode(self, jpeg_buf, element=None, border: str = "constant", quality: int = 85,
              jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.erode(decode(jpeg_buf), element))`` on the GPU, the pixels never leaving it.
        ``element`` and ``border`` as for ``vfilter.erode``; each channel of the decoded BGR frame on
        its own."""
        return self.filter_batch([jpeg_buf], Rank.erode(element, border), quality, jpeg_subsample, flags)[0]

    def erode_batch(self, jpeg_bufs: Sequence, element=None, border: str = "constant", quality: int = 85,
                    jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Rank.erode(element, border), quality, jpeg_subsample, flags)

    def dilate(self, jpeg_buf, element=None, border: str = "constant", quality: int = 85,
               jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.dilate(decode(jpeg_buf), element))`` on the GPU."""
        return self.filter_batch([jpeg_buf], Rank.dilate(element, border), quality, jpeg_subsample, flags)[0]

    def dilate_batch(self, jpeg_bufs: Sequence, element=None, border: str = "constant", quality: int = 85,
                     jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Rank.dilate(element, border), quality, jpeg_subsample, flags)

    def median_blur(self, jpeg_buf, ksize: int, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                    flags: int = 0) -> bytes:
        """``encode(cv2.medianBlur(decode(jpeg_buf), ksize))`` on the GPU; ``ksize`` 3 or 5."""
        return self.filter_batch([jpeg_buf], Rank.median(ksize), quality, jpeg_subsample, flags)[0]

    def median_blur_batch(self, jpeg_bufs: Sequence, ksize: int, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                          flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Rank.median(ksize), quality, jpeg_subsample, flags)

    # -- a colour matrix: cv2.transform between decode and encode ---------------------------------------
    # The submit forms go through ``filter_batch_submit*`` with a ``vfilter.filters.Mix``.
    def transform(self, jpeg_buf, m, rounding: str = "half_even", quality: int = 85,
                  jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.transform(decode(jpeg_buf), m))`` on the GPU, the pixels never leaving it.  ``m``
        and ``rounding`` as for ``vfilter.transform``; the matrix sees the decoded BGR pixel (channel 0
        is blue)."""
        return self.filter_batch([jpeg_buf], _as_mix("transform", m, rounding), quality, jpeg_subsample, flags)[0]

    def transform_batch(self, jpeg_bufs: Sequence, m, rounding: str = "half_even", quality: int = 85,
                        jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, _as_mix("transform_batch", m, rounding), quality, jpeg_subsample, flags)

    # -- a separable filter: cv2.sepFilter2D / cv2.blur between decode and encode --------------------------
    # The submit forms go through ``filter_batch_submit*`` with a ``vfilter.filters.Separable``.
    @staticmethod
    def _as_sep(kx, ky, shift, divisor, rounding, border) -> Separable:
        if not isinstance(kx, Separable):
            return Separable(kx, ky, shift, divisor, rounding, border)
        if ky is not None or shift is not None or divisor is not None:
            raise ValueError("sep_filter2d: a Separable carries its own taps and scale")
        return kx

    def sep_filter2d(self, jpeg_buf, kx, ky=None, shift=None, divisor=None, rounding: str = "half_even",
                     border: str = "reflect101", quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                     flags: int = 0) -> bytes:
        """``encode(cv2.sepFilter2D(decode(jpeg_buf), -1, kx, ky))`` on the GPU, the pixels never leaving it.
        The filter arguments as for ``vfilter.sep_filter2d`` (``kx`` may be a ``Separable``); the taps are
        applied to each channel of the decoded BGR frame."""
        return self.filter_batch([jpeg_buf], self._as_sep(kx, ky, shift, divisor, rounding, border), quality,
                                 jpeg_subsample, flags)[0]

    def sep_filter2d_batch(self, jpeg_bufs: Sequence, kx, ky=None, shift=None, divisor=None,
                           rounding: str = "half_even", border: str = "reflect101", quality: int = 85,
                           jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, self._as_sep(kx, ky, shift, divisor, rounding, border), quality,
                                 jpeg_subsample, flags)

    def blur(self, jpeg_buf, ksize, border: str = "reflect101", quality: int = 85, jpeg_subsample: int = TJSAMP_422,
             flags: int = 0) -> bytes:
        """``encode(cv2.blur(decode(jpeg_buf), ksize))`` on the GPU; ``ksize`` as for ``vfilter.blur``."""
        return self.filter_batch([jpeg_buf], Separable.box(ksize, True, border), quality, jpeg_subsample, flags)[0]

    def blur_batch(self, jpeg_bufs: Sequence, ksize, border: str = "reflect101", quality: int = 85,
                   jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Separable.box(ksize, True, border), quality, jpeg_subsample, flags)

    # -- the level filter: cv2.equalizeHist / auto-levels between decode and encode ------------------------
    # The submit forms go through ``filter_batch_submit*`` with a ``vfilter.filters.Level``.
    def equalize_hist(self, jpeg_buf, quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(equalize(decode(jpeg_buf)))`` on the GPU, the pixels never leaving it: every channel of the
        decoded BGR frame through ``cv2.equalizeHist`` by its own histogram."""
        return self.filter_batch([jpeg_buf], Level.equalize(), quality, jpeg_subsample, flags)[0]

    def equalize_hist_batch(self, jpeg_bufs: Sequence, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                            flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Level.equalize(), quality, jpeg_subsample, flags)

    def auto_levels(self, jpeg_buf, clip=0.0, link: bool = False, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                    flags: int = 0) -> bytes:
        """``encode(vfilter.auto_levels(decode(jpeg_buf), clip, link))`` on the GPU."""
        return self.filter_batch([jpeg_buf], Level.stretch(clip, None, link), quality, jpeg_subsample, flags)[0]

    def auto_levels_batch(self, jpeg_bufs: Sequence, clip=0.0, link: bool = False, quality: int = 85,
                          jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Level.stretch(clip, None, link), quality, jpeg_subsample, flags)

    # -- CLAHE (cv2.createCLAHE(...).apply) between decode and encode -------------------------------------
    # The submit forms go through ``filter_batch_submit*`` with a ``vfilter.filters.Clahe``.
    def clahe(self, jpeg_buf, clip_limit=40.0, tile_grid_size=(8, 8), channels=None, quality: int = 85,
              jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(vfilter.clahe(decode(jpeg_buf), clip_limit, tile_grid_size, channels))`` on the GPU, the pixels
        never leaving it: every filtered channel of the decoded BGR frame on its own."""
        return self.filter_batch([jpeg_buf], Clahe(clip_limit, tile_grid_size, channels), quality, jpeg_subsample, flags)[0]

    def clahe_batch(self, jpeg_bufs: Sequence, clip_limit=40.0, tile_grid_size=(8, 8), channels=None, quality: int = 85,
                    jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Clahe(clip_limit, tile_grid_size, channels), quality, jpeg_subsample, flags)

    # -- the affine warp (cv2.warpAffine, cv2.flip) between decode and encode ---------------------------------
    # The batch and submit forms go through ``filter_batch*`` with a ``vfilter.filters.Warp``.
    def warp_affine(self, jpeg_buf, M, flags="linear", border: str = "constant", border_value=0, inverse_map: bool = False,
                    quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags_tj: int = 0) -> bytes:
        """``encode(vfilter.warp_affine(decode(jpeg_buf), M, ...))`` on the GPU, the pixels never leaving it; the
        frame keeps its size.  ``flags`` as ``vfilter.warp_affine``'s; ``flags_tj``: the TurboJPEG flags."""
        interpolation, inverse = _warp_flags(flags, inverse_map)
        return self.filter_batch([jpeg_buf], Warp(M, None, interpolation, border, border_value, inverse), quality,
                                 jpeg_subsample, flags_tj)[0]

    def flip(self, jpeg_buf, code, quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.flip(decode(jpeg_buf), code))`` on the GPU: ``code`` 0, 1, -1 or "v", "h", "both"."""
        if isinstance(code, (int, np.integer)) and not isinstance(code, (bool, np.bool_)):
            code = 1 if code > 0 else -1 if code < 0 else 0
        return self.filter_batch([jpeg_buf], Warp(flip=code, interpolation="nearest"), quality, jpeg_subsample, flags)[0]

    # -- the resize (cv2.resize): the result is a JPEG of another size ------------------------------------
    def resize(self, jpeg_buf, dsize=None, fx=0, fy=0, interpolation="linear", quality: int = 85,
               jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(vfilter.resize(decode(jpeg_buf), dsize, fx, fy, interpolation))`` on the GPU, the pixels never
        leaving it; the JPEG's header carries the result's size."""
        return self.filter_batch([jpeg_buf], Resize(dsize, fx, fy, interpolation), quality, jpeg_subsample, flags)[0]

    def resize_batch(self, jpeg_bufs: Sequence, dsize=None, fx=0, fy=0, interpolation="linear", quality: int = 85,
                     jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> List[bytes]:
        """``resize`` over a batch of mixed input sizes in one GPU pass; with ``fx``, ``fy`` each from its own size."""
        return self.filter_batch(jpeg_bufs, Resize(dsize, fx, fy, interpolation), quality, jpeg_subsample, flags)

    # -- a filter chain (vfilter.filters.Chain) between one decode and one encode ------------------------
    def chain(self, jpeg_buf, chain, quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(run(decode(jpeg_buf), chain))`` on the GPU with one decode and one encode: the steps
        in between see the pixels, not JPEG generations.  ``chain`` is a ``Chain`` or a list of steps,
        as for ``vfilter.chain``; every step works on the decoded BGR frame."""
        return self.filter_batch([jpeg_buf], _as_chain(chain), quality, jpeg_subsample, flags)[0]

    def chain_batch(self, jpeg_bufs: Sequence, chain, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                    flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, _as_chain(chain), quality, jpeg_subsample, flags)

    def chain_batch_submit(self, jpeg_bufs: Sequence, chain, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                           flags: int = 0) -> int:
        """The program is copied, with its tables, kernels and elements: the caller may change them at once."""
        return self.filter_batch_submit(jpeg_bufs, _as_chain(chain), quality, jpeg_subsample, flags)

    def chain_batch_submit_addrs(self, addrs, sizes, chain, quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                                 flags: int = 0) -> int:
        return self.filter_batch_submit_addrs(addrs, sizes, _as_chain(chain), quality,
                                              jpeg_subsample, flags)

    def morphology_ex(self, jpeg_buf, op: str, element=None, iterations: int = 1, border: str = "constant",
                      quality: int = 85, jpeg_subsample: int = TJSAMP_422, flags: int = 0) -> bytes:
        """``encode(cv2.morphologyEx(decode(jpeg_buf), op, element, iterations=iterations))`` on the GPU;
        the arguments as for ``vfilter.morphology_ex``."""
        return self.filter_batch([jpeg_buf], Morph(op, element, iterations, border), quality, jpeg_subsample, flags)[0]

    def morphology_ex_batch(self, jpeg_bufs: Sequence, op: str, element=None, iterations: int = 1,
                            border: str = "constant", quality: int = 85, jpeg_subsample: int = TJSAMP_422,
                            flags: int = 0) -> List[bytes]:
        return self.filter_batch(jpeg_bufs, Morph(op, element, iterations, border), quality, jpeg_subsample, flags)

    def invert_batch_result_into_addrs(self, ticket: int, out_addrs, cap: int):
        """(sizes, {i: JPEG that did not fit}): each result written at ``out_addrs[i]`` (``cap``
        writable bytes each) when it fits there."""
        return self.ctx.jpeg_invert_result_into_addrs(ticket, out_addrs, cap)

    def invert_batch_ready(self, ticket: int) -> bool:
        return self.ctx.jpeg_invert_ready(ticket)

    def invert_batch_result(self, ticket: int) -> List[np.ndarray]:
        """The inverted JPEGs of a submitted batch (bytes-like uint8 views), in batch order."""
        return self.ctx.jpeg_invert_result(ticket)

    def invert_batch_result_into(self, ticket: int, outs: Sequence) -> List[np.ndarray]:
        """The same, each JPEG written straight into ``outs[i]`` when it fits there (e.g. the
        output half of its ring slot); a frame without room comes back in a fresh buffer."""
        return self.ctx.jpeg_invert_result_into(ticket, outs)
