"""The filter entry points: ``cv2.bitwise_not`` semantics on the MI355X.

Reference call site: ``inverted = cv2.bitwise_not(frame)`` (inverter.py:41), frame a
C-contiguous uint8 H x W x 3 ndarray (a read-only view from ``np.frombuffer`` on the raw
path, inverter.py:34).  ``bitwise_not`` keeps that signature: a new same-shape, same-dtype
array comes back and the input is never written.  The work runs in libvfilter_hip.so;
there is no CPU fallback.
"""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional, Sequence

import numpy as np

from ._lib import Context, get_context

_PINNED_RESULTS = os.environ.get("VF_PINNED_RESULTS", "1") != "0"


def bitwise_not(src: np.ndarray, dst: Optional[np.ndarray] = None, mask=None,
                ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.bitwise_not(src[, dst[, mask]])`` (inverter.py:41).

    Per-element bitwise NOT over the raw bytes of ``src`` (any dtype, any shape; the
    reference passes uint8 H x W x 3).  ``dst`` (optional) receives the result and is
    returned; it must have ``src``'s shape and dtype.  ``mask`` is not supported (the
    reference never passes one) and raises.
    """
    if mask is not None:
        raise NotImplementedError("bitwise_not: mask is not supported (inverter.py:41 passes none)")
    src = np.ascontiguousarray(src)
    ctx = ctx or get_context()
    if dst is None:
        # a result in the context's pinned arena: the kernel writes it directly over PCIe
        # (no staging copy out); it goes back to the arena when the array is dropped.  Past the
        # arena's cap of live results (VF_PINNED_RESULT_CAP, 1 GiB), when page-locking fails, or
        # with VF_PINNED_RESULTS=0, the result is an ordinary array, as cv2.bitwise_not's is
        dst = ctx._arena.try_empty(src.shape, src.dtype) if _PINNED_RESULTS else None
        if dst is None:
            dst = np.empty_like(src)
    elif dst.shape != src.shape or dst.dtype != src.dtype or not dst.flags.c_contiguous:
        raise ValueError("bitwise_not: dst must be C-contiguous with src's shape and dtype")
    ctx.invert_host(src, dst, src.nbytes)
    return dst


invert = bitwise_not


def invert_bytes(frame_bytes, ctx: Optional[Context] = None) -> bytes:
    """bytes -> inverted bytes (inverter.py:34 -> :41 -> :46 without the fixed reshape)."""
    src = np.frombuffer(frame_bytes, dtype=np.uint8)
    out = bytearray(src.nbytes)
    if src.nbytes:
        (ctx or get_context()).invert_host(src, np.frombuffer(out, dtype=np.uint8), src.nbytes)
    return bytes(out)


def invert_batch(frames: np.ndarray, out: Optional[np.ndarray] = None,
                 ctx: Optional[Context] = None) -> np.ndarray:
    """Invert a packed (N, H, W, 3) batch in one pipelined pass (replaces N iterations of
    worker.py:57 -> inverter.py:41)."""
    frames = np.ascontiguousarray(frames)
    if out is None:
        out = np.empty_like(frames)
    n = frames.shape[0] if frames.ndim else 1
    fb = frames.nbytes // max(n, 1)
    (ctx or get_context()).invert_batch_host(frames, out, fb, n)
    return out


_TABLE_SHAPES_1 = ((256,), (256, 1), (1, 256))
_TABLE_SHAPES_3 = ((256, 3), (256, 1, 3), (1, 256, 3))


def as_table(table) -> tuple:
    """A ``cv2.LUT`` table in the library's layout: ``(planar bytes, channels)``.

    ``table`` is uint8 with 256 elements -- shape (256,), (256, 1) or (1, 256) -- or 768 with
    the channel as the last axis -- (256, 3), (256, 1, 3) or (1, 256, 3).  The result holds
    ``channels`` tables of 256 bytes back to back: ``planar[c * 256 + v] == table[v, c]``.
    Anything else raises ``ValueError``.
    """
    t = np.asarray(table)
    if t.dtype != np.uint8:
        raise ValueError(f"lut: the table must be uint8, not {t.dtype}")
    if t.shape in _TABLE_SHAPES_1:
        return t.reshape(256).tobytes(), 1
    if t.shape in _TABLE_SHAPES_3:
        return np.ascontiguousarray(t.reshape(256, 3).T).tobytes(), 3
    raise ValueError(f"lut: a table has 256 entries for 1 or 3 channels, not shape {t.shape}")


def lut(src: np.ndarray, table, dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.LUT(src, lut[, dst])`` on uint8 input: ``dst[i] = table[src[i]]``, with a
    3-channel table each channel of an ``... x 3`` ``src`` through its own.  Any other filter a
    plugin puts at inverter.py:41 -- ``vfilter.tables`` builds the usual ones."""
    planar, channels = as_table(table)
    if not isinstance(src, np.ndarray) or src.dtype != np.uint8:
        raise ValueError("lut: src must be a uint8 ndarray")
    if channels == 3 and (src.ndim < 1 or src.shape[-1] != 3):
        raise ValueError(f"lut: a 3-channel table needs src.shape[-1] == 3, not shape {src.shape}")
    src = np.ascontiguousarray(src)
    if dst is None:
        dst = np.empty_like(src)
    elif dst.shape != src.shape or dst.dtype != src.dtype or not dst.flags.c_contiguous:
        raise ValueError("lut: dst must be C-contiguous with src's shape and dtype")
    (ctx or get_context()).lut_frames_host([src], [dst], [src.nbytes], planar, channels)
    return dst


def lut_frames(frames: Sequence, table, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """``lut`` over separately stored frames (uint8 ndarrays or bytes-likes; mixed sizes allowed) in
    one call.  With a 3-channel table every frame is interleaved 3-channel data from channel 0.
    Returns ndarrays (or fills ``outs``)."""
    planar, channels = as_table(table)
    srcs = [np.ascontiguousarray(f) if isinstance(f, np.ndarray) else np.frombuffer(f, dtype=np.uint8)
            for f in frames]
    for s in srcs:
        if s.dtype != np.uint8:
            raise ValueError("lut_frames: frames must be uint8")
        if channels == 3 and s.nbytes % 3:
            raise ValueError("lut_frames: a 3-channel table needs frames of whole 3-byte pixels")
    if outs is None:
        outs = [np.empty_like(s) for s in srcs]
    (ctx or get_context()).lut_frames_host(srcs, outs, [s.nbytes for s in srcs], planar, channels)
    return outs


BORDERS = {"reflect101": 0, "replicate": 1, "constant": 2}  # VF_BORDER_* (include/vfilter.h)


def border_code(border) -> int:
    """``border`` ("reflect101", the default of cv2.filter2D; "replicate"; "constant", with the
    constant 0) as the library's code."""
    try:
        return BORDERS[border]
    except (KeyError, TypeError):
        raise ValueError(f"filter2d: border must be one of {sorted(BORDERS)}, not {border!r}") from None


def as_kernel(kernel) -> tuple:
    """A ``cv2.filter2D`` kernel in the library's form: ``(int16 kh x kw weights, shift)``, meaning
    ``weights / 2**shift``, with the smallest such shift.

    ``kernel`` is a 2-D integer array (shift 0), a ``(weights, shift)`` pair (``vfilter.kernels``
    builds those), or a 2-D floating-point array that is *dyadic*: ``kernel * 2**s`` is integral for
    some s in 0..16.  Sides are odd and at most 7, ``0 <= shift <= 16`` and ``sum|weights| <= 65536``.
    Anything else -- a 1/9 mean, a sampled Gaussian -- raises ``ValueError`` with the reason: there is
    no floating-point kernel path."""
    shift = 0
    if isinstance(kernel, tuple) and len(kernel) == 2 and np.ndim(kernel[1]) == 0 and np.ndim(kernel[0]) == 2:
        kernel, shift = kernel
        if int(shift) != shift:
            raise ValueError(f"filter2d: shift must be an integer, not {shift!r}")
        shift = int(shift)
        k = np.asarray(kernel)
        if k.dtype.kind not in "iub":
            if k.dtype.kind != "f" or not np.array_equal(k, np.rint(k)):
                raise ValueError("filter2d: the weights of a (weights, shift) pair must be integers")
    else:
        k = np.asarray(kernel)
    if k.ndim != 2 or k.size == 0:
        raise ValueError(f"filter2d: a kernel is a 2-D array, not shape {k.shape}")
    kh, kw = k.shape
    if kh % 2 == 0 or kw % 2 == 0 or kh > 7 or kw > 7:
        raise ValueError(f"filter2d: a {kh} x {kw} kernel; sides must be odd and at most 7")
    if not 0 <= shift <= 16:
        raise ValueError(f"filter2d: shift = {shift} outside 0..16")
    if k.dtype.kind == "f" and not np.array_equal(k, np.rint(k)):
        if not np.isfinite(k).all():
            raise ValueError("filter2d: the kernel has a non-finite weight")
        k = k.astype(np.float64)
        for s in range(1, 17):
            scaled = k * float(1 << s)  # exact: a power of two
            if np.array_equal(scaled, np.rint(scaled)):
                k, shift = scaled, s
                break
        else:
            raise ValueError("filter2d: the kernel is not dyadic (no s in 0..16 makes kernel * 2**s integral); "
                             "give integer weights and a shift")
    elif k.dtype.kind not in "iubf":
        raise ValueError(f"filter2d: a kernel of dtype {k.dtype}")
    w = np.asarray(np.rint(k) if k.dtype.kind == "f" else k).astype(np.int64)
    while shift > 0 and not (w & 1).any():  # the smallest shift
        w >>= 1
        shift -= 1
    total = int(np.abs(w).sum())
    if total > 65536:
        raise ValueError(f"filter2d: sum|weights| = {total} exceeds 65536")
    if w.size and (int(w.max()) > 32767 or int(w.min()) < -32768):
        raise ValueError("filter2d: a weight does not fit 16 bits")
    return np.ascontiguousarray(w, dtype=np.int16), shift


# -- a batch's filter as one value (TurboJPEG.filter_*, the workers) ------------------------------
# Immutable and validated when constructed, so a bad table or kernel is refused before any GPU
# work.  ``family`` names the methods the value goes through -- ``Context.jpeg_<family>``,
# ``jpeg_<family>_submit``, ``jpeg_<family>_submit_addrs`` -- and ``args`` are the arguments those
# take between the batch and the quality.  This is the one place that pairs the two.

@dataclasses.dataclass(frozen=True)
class Invert:
    """``cv2.bitwise_not`` (inverter.py:41)."""
    family = "invert"
    args = ()


@dataclasses.dataclass(frozen=True, init=False)
class Table:
    """``cv2.LUT`` with ``table`` (as for ``lut``), copied: the caller may change its array at once."""
    planar: bytes
    channels: int
    family = "lut"

    def __init__(self, table):
        planar, channels = as_table(table)
        object.__setattr__(self, "planar", planar)
        object.__setattr__(self, "channels", channels)

    @property
    def args(self) -> tuple:
        return self.planar, self.channels


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Kernel:
    """``cv2.filter2D`` with ``kernel`` and ``border`` (as for ``filter2d``), copied."""
    weights: np.ndarray  # int16 kh x kw, read-only
    shift: int
    border: str
    border_code: int
    family = "conv"

    def __init__(self, kernel, border: str = "reflect101"):
        weights, shift = as_kernel(kernel)
        weights.flags.writeable = False
        fields = {"weights": weights, "shift": shift, "border": border, "border_code": border_code(border)}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @property
    def args(self) -> tuple:
        return self.weights, self.shift, self.border_code


def _conv_frame(name: str, a) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise ValueError(f"{name}: frames must be uint8 ndarrays")
    if a.ndim == 3 and a.shape[2] in (1, 3):
        return a
    if a.ndim == 2:
        return a
    raise ValueError(f"{name}: a frame is H x W or H x W x 3, not shape {a.shape}")


def _frames_call(name: str, srcs: List[np.ndarray], outs: Optional[List], call) -> List:
    """The frame-list work of ``filter2d_frames``, ``rank_frames`` and ``chain_frames`` (``name``, for the
    messages) on checked frames: one channel count, ``outs`` made or checked, and
    ``call(srcs, outs, widths, heights, channels)`` on the frames that are not empty."""
    srcs = [np.ascontiguousarray(s) for s in srcs]
    chans = {1 if s.ndim == 2 else s.shape[2] for s in srcs}
    if len(chans) > 1:
        raise ValueError(f"{name}: the frames of one call have one channel count")
    if outs is None:
        outs = [np.empty_like(s) for s in srcs]
    elif len(outs) != len(srcs) or any(o.shape != s.shape or o.dtype != np.uint8 or not o.flags.c_contiguous
                                       for o, s in zip(outs, srcs)):
        raise ValueError(f"{name}: outs must be C-contiguous uint8 arrays of the frames' shapes")
    live = [(s, o) for s, o in zip(srcs, outs) if s.size]
    if live:
        call([s for s, _ in live], [o for _, o in live], [s.shape[1] for s, _ in live],
             [s.shape[0] for s, _ in live], chans.pop())
    return outs


def filter2d(src: np.ndarray, kernel, dst: Optional[np.ndarray] = None, border: str = "reflect101",
             ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.filter2D(src, -1, kernel)`` on uint8 ``H x W`` or ``H x W x 3`` input
    (correlation, anchor at the centre, ``borderType`` reflect-101 by default), exact for the
    kernels ``as_kernel`` accepts.  ``dst`` as for ``lut``; it may not be ``src`` (the filter reads
    neighbours).  ``vfilter.kernels`` builds the usual kernels."""
    weights, shift = as_kernel(kernel)
    code = border_code(border)
    src = np.ascontiguousarray(_conv_frame("filter2d", src))
    dst = _rank_dst("filter2d", src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).conv_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, weights, shift,
                                                code)
    return dst


def filter2d_frames(frames: Sequence, kernel, outs: Optional[List] = None, border: str = "reflect101",
                    ctx: Optional[Context] = None) -> List:
    """``filter2d`` over separately stored frames of one channel count and mixed sizes in one call.
    Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    weights, shift = as_kernel(kernel)
    code = border_code(border)
    return _frames_call("filter2d_frames", [_conv_frame("filter2d_frames", f) for f in frames], outs,
                        lambda *a: (ctx or get_context()).conv_frames_host(*a, weights, shift, code))


# -- rank filters: cv2.erode, cv2.dilate, cv2.medianBlur ------------------------------------------

RANK_OPS = {"erode": 0, "dilate": 1, "median": 2}  # VF_RANK_* (include/vfilter.h)


def as_element(element=None) -> np.ndarray:
    """A structuring element in the library's form: a C-contiguous uint8 ``kh x kw`` array of 0 and 1.

    ``element`` is a 2-D array of integers, booleans or integral floats whose non-zero entries are
    the members; sides are odd and at most 7 and at least one entry is a member.  ``None`` is the
    3 x 3 rectangle, as cv2's empty kernel is.  Anything else raises ``ValueError``.
    ``vfilter.elements`` builds the usual ones."""
    if element is None:
        return np.ones((3, 3), np.uint8)
    e = np.asarray(element)
    if e.ndim != 2 or e.size == 0:
        raise ValueError(f"a structuring element is a 2-D array, not shape {e.shape}")
    kh, kw = e.shape
    if kh % 2 == 0 or kw % 2 == 0 or kh > 7 or kw > 7:
        raise ValueError(f"a {kh} x {kw} structuring element; sides must be odd and at most 7")
    if e.dtype.kind == "f":
        if not np.array_equal(e, np.rint(e)):
            raise ValueError("a structuring element holds integers (non-zero: member)")
    elif e.dtype.kind not in "iub":
        raise ValueError(f"a structuring element of dtype {e.dtype}")
    out = np.ascontiguousarray(e != 0, dtype=np.uint8)
    if not out.any():
        raise ValueError("a structuring element needs at least one member")
    return out


def _rank_border(name: str, border) -> int:
    try:
        return BORDERS[border]
    except (KeyError, TypeError):
        raise ValueError(f"{name}: border must be one of {sorted(BORDERS)}, not {border!r}") from None


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Rank:
    """``cv2.erode``, ``cv2.dilate`` or ``cv2.medianBlur`` as a batch's filter; build one with
    ``Rank.erode``, ``Rank.dilate`` or ``Rank.median``.  The element is copied."""
    op: str
    op_code: int
    element: np.ndarray  # uint8 0/1 kh x kw, read-only
    border: str
    border_code: int
    family = "rank"

    def __init__(self, op: str, element=None, border: str = "constant"):
        if op not in RANK_OPS:
            raise ValueError(f"rank: op must be one of {sorted(RANK_OPS)}, not {op!r}")
        e = as_element(element).copy()
        if op == "median":
            if e.shape not in ((3, 3), (5, 5)) or not e.all():
                raise ValueError("median: the full 3 x 3 or 5 x 5 square only")
            if border != "replicate":
                raise ValueError("median: cv2.medianBlur replicates the border; there is no other")
        e.flags.writeable = False
        fields = {"op": op, "op_code": RANK_OPS[op], "element": e, "border": border,
                  "border_code": _rank_border(op, border)}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @classmethod
    def erode(cls, element=None, border: str = "constant") -> "Rank":
        return cls("erode", element, border)

    @classmethod
    def dilate(cls, element=None, border: str = "constant") -> "Rank":
        return cls("dilate", element, border)

    @classmethod
    def median(cls, ksize: int) -> "Rank":
        if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)) or ksize not in (3, 5):
            raise ValueError(f"median_blur: ksize must be 3 or 5, not {ksize!r}")
        return cls("median", np.ones((ksize, ksize), np.uint8), "replicate")

    @property
    def args(self) -> tuple:
        return self.op_code, self.element, self.border_code


def _rank_dst(name: str, src: np.ndarray, dst) -> np.ndarray:
    if dst is None:
        return np.empty_like(src)
    if not isinstance(dst, np.ndarray) or dst.shape != src.shape or dst.dtype != src.dtype or not dst.flags.c_contiguous:
        raise ValueError(f"{name}: dst must be C-contiguous with src's shape and dtype")
    return dst


def _rank_one(name: str, src, rank: Rank, dst, ctx) -> np.ndarray:
    src = np.ascontiguousarray(_conv_frame(name, src))
    dst = _rank_dst(name, src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).rank_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *rank.args)
    return dst


def erode(src: np.ndarray, element=None, dst: Optional[np.ndarray] = None, border: str = "constant",
          ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.erode(src, element)`` on uint8 ``H x W`` or ``H x W x 3`` input: per channel
    the minimum over the element's members, anchor at the centre, one iteration.  ``element`` as for
    ``as_element`` (``None``: the 3 x 3 rectangle).  ``border`` "constant", the default, is cv2's
    default border: a tap outside the frame is left out of the minimum -- unlike ``filter2d``, where
    the constant is 0; "reflect101" and "replicate" read the frame as ``filter2d`` does.  ``dst`` as
    for ``filter2d``; it may not be ``src``."""
    return _rank_one("erode", src, Rank.erode(element, border), dst, ctx)


def dilate(src: np.ndarray, element=None, dst: Optional[np.ndarray] = None, border: str = "constant",
           ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.dilate(src, element)``: ``erode`` with the maximum (the element is not
    reflected, as in cv2).  ``border`` "constant", the default, leaves a tap outside the frame out of
    the maximum -- unlike ``filter2d``, where the constant is 0 (for the maximum of uint8 the two
    agree unless no tap of the element lands in the frame)."""
    return _rank_one("dilate", src, Rank.dilate(element, border), dst, ctx)


def median_blur(src: np.ndarray, ksize: int, dst: Optional[np.ndarray] = None,
                ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.medianBlur(src, ksize)`` on uint8 ``H x W`` or ``H x W x 3`` input, ``ksize``
    3 or 5: per channel the median of the ``ksize x ksize`` square, the border replicated (cv2 offers
    no other).  ``dst`` as for ``filter2d``."""
    return _rank_one("median_blur", src, Rank.median(ksize), dst, ctx)


def rank_frames(frames: Sequence, rank: Rank, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Rank`` filter over separately stored frames of one channel count and mixed sizes in one
    call.  Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    if not isinstance(rank, Rank):
        raise ValueError("rank_frames: rank is a vfilter.Rank (Rank.erode, Rank.dilate, Rank.median)")
    return _frames_call("rank_frames", [_conv_frame("rank_frames", f) for f in frames], outs,
                        lambda *a: (ctx or get_context()).rank_frames_host(*a, *rank.args))


# -- colour matrix: cv2.transform --------------------------------------------------------------------

ROUNDINGS = {"half_even": 0, "half_up": 1}  # VF_ROUND_* (include/vfilter.h)


def rounding_code(rounding) -> int:
    """``rounding`` ("half_even", cv2's float path; "half_up", ``(x + half) >> shift``, its fixed-point
    paths) as the library's code."""
    try:
        return ROUNDINGS[rounding]
    except (KeyError, TypeError):
        raise ValueError(f"transform: rounding must be one of {sorted(ROUNDINGS)}, not {rounding!r}") from None


def as_matrix(m) -> tuple:
    """A ``cv2.transform`` matrix in the library's form: ``(int32 3 x 4 [M | t], shift)``, meaning
    ``[M | t] / 2**shift``, with the smallest such shift.

    ``m`` is a 3 x 3 or 3 x 4 integer array (shift 0; a 3 x 3 has offset 0), an ``(ints, shift)`` pair
    (``vfilter.colors`` builds those), or a floating-point array that is *dyadic*: ``m * 2**s`` is
    integral for some s in 0..16.  Every weight fits int16, ``sum|M[c]| <= 65536`` per row,
    ``0 <= shift <= 16`` and the offsets, scaled by ``2**shift``, have ``|t[c]| <= 255 * 2**shift``.
    Anything else -- the Rec. 601 luma as floats, a non-finite entry -- raises ``ValueError`` with the
    reason: there is no floating-point matrix path."""
    shift = 0
    if isinstance(m, tuple) and len(m) == 2 and np.ndim(m[1]) == 0 and np.ndim(m[0]) == 2:
        m, shift = m
        if int(shift) != shift:
            raise ValueError(f"transform: shift must be an integer, not {shift!r}")
        shift = int(shift)
        k = np.asarray(m)
        if k.dtype.kind not in "iub":
            if k.dtype.kind != "f" or not np.array_equal(k, np.rint(k)):
                raise ValueError("transform: the entries of an (ints, shift) pair must be integers")
    else:
        k = np.asarray(m)
    if k.shape not in ((3, 3), (3, 4)):
        raise ValueError(f"transform: a matrix is 3 x 3 or 3 x 4, not shape {k.shape}")
    if not 0 <= shift <= 16:
        raise ValueError(f"transform: shift = {shift} outside 0..16")
    if k.dtype.kind == "f" and not np.array_equal(k, np.rint(k)):
        if not np.isfinite(k).all():
            raise ValueError("transform: the matrix has a non-finite entry")
        k = k.astype(np.float64)
        for s in range(1, 17):
            scaled = k * float(1 << s)  # exact: a power of two
            if np.array_equal(scaled, np.rint(scaled)):
                k, shift = scaled, s
                break
        else:
            raise ValueError("transform: the matrix is not dyadic (no s in 0..16 makes m * 2**s integral); "
                             "give integers and a shift")
    elif k.dtype.kind not in "iubf":
        raise ValueError(f"transform: a matrix of dtype {k.dtype}")
    w = np.asarray(np.rint(k) if k.dtype.kind == "f" else k).astype(np.int64)
    if w.shape == (3, 3):
        w = np.concatenate([w, np.zeros((3, 1), np.int64)], axis=1)
    while shift > 0 and not (w & 1).any():  # the smallest shift
        w >>= 1
        shift -= 1
    if int(w[:, :3].max()) > 32767 or int(w[:, :3].min()) < -32768:
        raise ValueError("transform: a weight does not fit 16 bits")
    total = int(np.abs(w[:, :3]).sum(axis=1).max())
    if total > 65536:
        raise ValueError(f"transform: a row's sum|weights| = {total} exceeds 65536")
    most = 255 << shift
    if int(np.abs(w[:, 3]).max()) > most:
        raise ValueError(f"transform: an offset of {int(np.abs(w[:, 3]).max())} / 2**{shift} is outside -255..255")
    return np.ascontiguousarray(w, dtype=np.int32), shift


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Mix:
    """``cv2.transform`` with the 3 x 3 or 3 x 4 ``matrix`` (as for ``as_matrix``) and a rounding, copied:
    per pixel ``dst = clamp(round((M . src + t) / 2**shift))``.  ``rounding`` is "half_even" (cv2's float
    path) or "half_up" (``(x + half) >> shift``, cv2's fixed-point paths); with shift 0 there is nothing
    to round.  ``vfilter.colors`` builds the usual matrices.  3-channel frames only."""
    matrix: np.ndarray  # int32 3 x 4 [M | t], read-only
    shift: int
    rounding: str
    rounding_code: int
    family = "mix"

    def __init__(self, matrix, rounding: str = "half_even"):
        if isinstance(matrix, Mix):
            raise ValueError("Mix: matrix is a matrix or an (ints, shift) pair, not a Mix")
        code = rounding_code(rounding)
        m, shift = as_matrix(matrix)
        m.flags.writeable = False
        for name, v in (("matrix", m), ("shift", shift), ("rounding", rounding), ("rounding_code", code)):
            object.__setattr__(self, name, v)

    @property
    def args(self) -> tuple:
        return self.matrix, self.shift, self.rounding_code


def _as_mix(name: str, m, rounding: str) -> Mix:
    if not isinstance(m, Mix):
        return Mix(m, rounding)
    if rounding not in ("half_even", m.rounding):  # the default leaves a Mix its own rounding
        raise ValueError(f"{name}: the Mix rounds {m.rounding}; rounding={rounding!r} contradicts it")
    return m


def _mix_frame(name: str, a) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise ValueError(f"{name}: frames must be uint8 ndarrays")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{name}: a colour matrix mixes the 3 channels of a pixel; frames are H x W x 3, "
                         f"not shape {a.shape}")
    return a


def transform(src: np.ndarray, m, dst: Optional[np.ndarray] = None, rounding: str = "half_even",
              ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.transform(src, m)`` on uint8 ``H x W x 3`` input with a 3 x 3 or 3 x 4 ``m`` that
    ``as_matrix`` accepts (or a ``Mix``, which carries its rounding), exact in integers: grayscale
    kept in 3 channels, BGR <-> RGB, sepia, saturation, white balance, channel mixing
    (``vfilter.colors``).  ``dst`` as for ``lut``, and it may be ``src``.  1-channel frames are refused."""
    mix = _as_mix("transform", m, rounding)
    src = np.ascontiguousarray(_mix_frame("transform", src))
    dst = _rank_dst("transform", src, dst)
    if src.size:
        (ctx or get_context()).mix_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], 3, *mix.args)
    return dst


def transform_frames(frames: Sequence, mix, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Mix`` (or a matrix, as for ``transform``) over separately stored ``H x W x 3`` frames of mixed
    sizes in one call.  Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    mix = _as_mix("transform_frames", mix, "half_even")
    return _frames_call("transform_frames", [_mix_frame("transform_frames", f) for f in frames], outs,
                        lambda *a: (ctx or get_context()).mix_frames_host(*a, *mix.args))


# -- separable filter: cv2.sepFilter2D, cv2.blur, cv2.boxFilter -----------------------------------------

SEP_MAX_TAPS = 31  # per axis (csrc/vf_sep_plan.h kMaxSide)


def as_taps(k) -> tuple:
    """The taps of one axis of a separable kernel in the library's form: ``(int16 taps, shift)``, meaning
    ``taps / 2**shift``, with the smallest such shift.

    ``k`` is a 1-D integer array (shift 0), an ``(ints, shift)`` pair (``vfilter.kernels.binomial_taps`` and
    ``gaussian_taps`` build those), or a 1-D floating-point array that is *dyadic*, by ``as_kernel``'s
    rules.  The count is odd and at most 31, every tap fits int16, ``0 <= shift <= 16``.  Anything else
    raises ``ValueError`` with the reason."""
    shift = 0
    if isinstance(k, tuple) and len(k) == 2 and np.ndim(k[1]) == 0 and np.ndim(k[0]) == 1:
        k, shift = k
        if int(shift) != shift:
            raise ValueError(f"sep_filter2d: shift must be an integer, not {shift!r}")
        shift = int(shift)
        t = np.asarray(k)
        if t.dtype.kind not in "iub":
            if t.dtype.kind != "f" or not np.array_equal(t, np.rint(t)):
                raise ValueError("sep_filter2d: the taps of a (taps, shift) pair must be integers")
    else:
        t = np.asarray(k)
    if t.ndim != 1 or t.size == 0:
        raise ValueError(f"sep_filter2d: the taps of an axis are a 1-D array, not shape {t.shape}")
    if t.size % 2 == 0 or t.size > SEP_MAX_TAPS:
        raise ValueError(f"sep_filter2d: {t.size} taps; the count must be odd and at most {SEP_MAX_TAPS}")
    if not 0 <= shift <= 16:
        raise ValueError(f"sep_filter2d: shift = {shift} outside 0..16")
    if t.dtype.kind == "f" and not np.isfinite(t).all():
        raise ValueError("sep_filter2d: the taps have a non-finite entry")
    if t.dtype.kind == "f" and not np.array_equal(t, np.rint(t)):
        t = t.astype(np.float64)
        for s in range(1, 17):
            scaled = t * float(1 << s)  # exact: a power of two
            if np.array_equal(scaled, np.rint(scaled)):
                t, shift = scaled, s
                break
        else:
            raise ValueError("sep_filter2d: the taps are not dyadic (no s in 0..16 makes taps * 2**s integral); "
                             "give integer taps and a shift, or a divisor")
    elif t.dtype.kind not in "iubf":
        raise ValueError(f"sep_filter2d: taps of dtype {t.dtype}")
    w = np.asarray(np.rint(t) if t.dtype.kind == "f" else t).astype(np.int64)
    while shift > 0 and not (w & 1).any():  # the smallest shift
        w >>= 1
        shift -= 1
    if int(w.max()) > 32767 or int(w.min()) < -32768:
        raise ValueError("sep_filter2d: a tap does not fit 16 bits")
    return np.ascontiguousarray(w, dtype=np.int16), shift


def _sep_sides(name: str, ksize) -> tuple:
    """``ksize`` -- an int, or ``(width, height)`` in cv2's order -- as odd ``(kw, kh)`` of at most 31."""
    try:
        kw, kh = (ksize, ksize) if np.ndim(ksize) == 0 else ksize
        if int(kw) != kw or int(kh) != kh:
            raise TypeError
        kw, kh = int(kw), int(kh)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: ksize is an int or (width, height), not {ksize!r}") from None
    if kw < 1 or kh < 1 or kw > SEP_MAX_TAPS or kh > SEP_MAX_TAPS or kw % 2 == 0 or kh % 2 == 0:
        raise ValueError(f"{name}: a {kw} x {kh} kernel; sides must be odd and at most {SEP_MAX_TAPS} "
                         "(an even side has no centre)")
    return kw, kh


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Separable:
    """``cv2.sepFilter2D`` with the horizontal taps ``kx`` and the vertical taps ``ky`` (each as for
    ``as_taps``; ``ky=None``: ``kx``), copied: ``dst = clamp(round(sum_j ky[j] sum_i kx[i] src / scale))``, exact in
    integers, with one rounding at the end.  The scale is ``2**shift`` -- the shifts of the two axes
    and ``shift`` add up, to at most 16, and the smallest common shift is taken -- rounded
    ``rounding`` ("half_even", cv2's float path; "half_up", ``(x + half) >> shift``, cv2's 8-bit fixed-point
    path), or the odd ``divisor`` (at most 1023, to nearest: no tie exists), not both.
    ``sum|kx| * sum|ky| <= 65536``.  ``Separable.box`` is ``cv2.blur`` / ``cv2.boxFilter``, ``Separable.gaussian``
    a fixed-point Gaussian."""
    kx: np.ndarray  # int16, read-only
    ky: np.ndarray
    shift: int
    divisor: int
    rounding: str
    rounding_code: int
    border: str
    border_code: int
    family = "sep"

    def __init__(self, kx, ky=None, shift=None, divisor=None, rounding: str = "half_even",
                 border: str = "reflect101"):
        if isinstance(kx, Separable) or isinstance(ky, Separable):
            raise ValueError("Separable: kx and ky are taps, not a Separable")
        code = rounding_code(rounding)
        bcode = border_code(border)
        tx, sx = as_taps(kx)
        ty, sy = (tx.copy(), sx) if ky is None else as_taps(ky)
        extra = 0
        if shift is not None:
            if isinstance(shift, bool) or int(shift) != shift or shift < 0:
                raise ValueError(f"Separable: shift = {shift!r} is not a non-negative integer")
            extra = int(shift)
        total = sx + sy + extra
        x, y = tx.astype(np.int64), ty.astype(np.int64)
        while total > 0 and (not (x & 1).any() or not (y & 1).any()):  # the smallest common shift
            if not (x & 1).any():
                x >>= 1
            else:
                y >>= 1
            total -= 1
        if total > 16:
            raise ValueError(f"Separable: the shifts add up to {total}; at most 16")
        d = 1 if divisor is None else divisor
        if isinstance(d, bool) or int(d) != d or d < 1 or d > 1023 or d % 2 == 0:
            raise ValueError(f"Separable: divisor = {divisor!r}; a divisor is odd and 1..1023")
        d = int(d)
        if d != 1 and total != 0:
            raise ValueError(f"Separable: a shift of {total} together with divisor = {d}; a filter scales by one of them")
        prod = int(np.abs(x).sum()) * int(np.abs(y).sum())
        if prod > 65536:
            raise ValueError(f"Separable: sum|kx| * sum|ky| = {prod} exceeds 65536")
        tx, ty = x.astype(np.int16), y.astype(np.int16)
        tx.flags.writeable = False
        ty.flags.writeable = False
        fields = {"kx": tx, "ky": ty, "shift": total, "divisor": d, "rounding": rounding, "rounding_code": code,
                  "border": border, "border_code": bcode}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @classmethod
    def box(cls, ksize, normalize: bool = True, border: str = "reflect101") -> "Separable":
        """``cv2.blur(src, ksize)`` / ``cv2.boxFilter(src, -1, ksize, normalize=...)``: all taps 1 and the divisor
        ``width * height`` (``normalize=False``: the saturating sum).  ``ksize`` is an int or ``(width, height)``;
        sides are odd, so the area is."""
        kw, kh = _sep_sides("box", ksize)
        return cls(np.ones(kw, np.int16), np.ones(kh, np.int16), divisor=kw * kh if normalize else None,
                   border=border)

    @classmethod
    def gaussian(cls, ksize, sigma, bits: int = 8, rounding: str = "half_up",
                 border: str = "reflect101") -> "Separable":
        """A Gaussian in fixed point: ``vfilter.kernels.gaussian_taps(side, sigma, bits)`` on each axis and one
        ``(x + half) >> 2 * bits`` at the end (the structure of cv2's 8-bit path; the taps are this project's
        quantisation, not cv2's).  ``ksize`` an int or ``(width, height)``, ``sigma`` a number or ``(sigma_x,
        sigma_y)``; ``bits <= 8``."""
        from .kernels import gaussian_taps
        kw, kh = _sep_sides("gaussian", ksize)
        sx, sy = (sigma, sigma) if np.ndim(sigma) == 0 else sigma
        if int(bits) != bits or not 1 <= bits <= 8:
            raise ValueError(f"gaussian: bits = {bits!r}; two axes of `bits` bits stay within 16, so 1..8")
        return cls(gaussian_taps(kw, sx, bits), gaussian_taps(kh, sy, bits), rounding=rounding, border=border)

    @property
    def args(self) -> tuple:
        return self.kx, self.ky, self.shift, self.divisor, self.rounding_code, self.border_code


def _sep_one(name: str, src, sep: Separable, dst, ctx) -> np.ndarray:
    src = np.ascontiguousarray(_conv_frame(name, src))
    if dst is src:
        raise ValueError(f"{name}: dst may not be src (the filter reads neighbours)")
    dst = _rank_dst(name, src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).sep_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *sep.args)
    return dst


def sep_filter2d(src: np.ndarray, kx, ky=None, shift=None, divisor=None, rounding: str = "half_even",
                 border: str = "reflect101", dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.sepFilter2D(src, -1, kx, ky)`` on uint8 ``H x W`` or ``H x W x 3`` input (correlation,
    anchor at the centre, reflect-101 by default), exact for what ``Separable`` accepts; ``kx`` may be a
    ``Separable`` (then the other filter arguments stay at their defaults).  It equals ``filter2d`` with
    ``outer(ky, kx)`` wherever both exist, with up to 31 taps an axis.  ``dst`` as for ``filter2d``: not ``src``."""
    if isinstance(kx, Separable):
        if ky is not None or shift is not None or divisor is not None:
            raise ValueError("sep_filter2d: a Separable carries its own taps and scale")
        sep = kx
    else:
        sep = Separable(kx, ky, shift, divisor, rounding, border)
    return _sep_one("sep_filter2d", src, sep, dst, ctx)


def blur(src: np.ndarray, ksize, border: str = "reflect101", dst: Optional[np.ndarray] = None,
         ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.blur(src, ksize)``: the mean over ``ksize`` (an int, or ``(width, height)``; odd sides up
    to 31), rounded to nearest."""
    return _sep_one("blur", src, Separable.box(ksize, True, border), dst, ctx)


def box_filter(src: np.ndarray, ksize, normalize: bool = True, border: str = "reflect101",
               dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.boxFilter(src, -1, ksize, normalize=normalize)``; ``normalize=False`` is the saturating
    sum."""
    return _sep_one("box_filter", src, Separable.box(ksize, normalize, border), dst, ctx)


def sep_frames(frames: Sequence, sep: Separable, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Separable`` over separately stored frames of one channel count and mixed sizes in one call.
    Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    if not isinstance(sep, Separable):
        raise ValueError("sep_frames: sep is a Separable")
    return _frames_call("sep_frames", [_conv_frame("sep_frames", f) for f in frames], outs,
                        lambda *a: (ctx or get_context()).sep_frames_host(*a, *sep.args))


# -- level filter: cv2.equalizeHist, auto-levels, and the histogram --------------------------------------

LEVEL_RULES = {"equalize": 0, "stretch": 1}  # VF_LEVEL_* (include/vfilter.h)
LEVEL_MAX_CLIP = 32767  # in units of 1 / 65536 of the pixels (csrc/vf_level_plan.h kMaxClip)


def _level_clip(clip) -> tuple:
    """``clip`` -- a fraction in ``[0, 0.5)``, or ``(lo, hi)`` of them -- as the two integer clips."""
    try:
        lo, hi = (clip, clip) if np.ndim(clip) == 0 else clip
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"Level: clip is a fraction or (lo, hi), not {clip!r}") from None
    out = []
    for f in (lo, hi):
        if not 0.0 <= f < 0.5:  # a NaN fails this too
            raise ValueError(f"Level: clip = {f!r}; a clip is a fraction in [0, 0.5)")
        q = int(round(f * 65536))
        if q > LEVEL_MAX_CLIP:
            raise ValueError(f"Level: clip = {f!r} is {q} / 65536; at most {LEVEL_MAX_CLIP} / 65536")
        out.append(q)
    return tuple(out)


def _level_mask(channels) -> int:
    """``channels`` -- ``None`` (all of the frame's) or channel indices among 0, 1, 2 -- as the mask's bits."""
    if channels is None:
        return 0
    try:
        chans = [channels] if np.ndim(channels) == 0 else list(channels)
        if any(isinstance(c, bool) or int(c) != c for c in chans):
            raise TypeError
        chans = [int(c) for c in chans]
    except (TypeError, ValueError):
        raise ValueError(f"Level: channels is None or channel indices, not {channels!r}") from None
    if not chans or any(c < 0 or c > 2 for c in chans) or len(set(chans)) != len(chans):
        raise ValueError(f"Level: channels = {channels!r}; distinct indices among 0, 1, 2, at least one")
    return sum(1 << c for c in chans)


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Level:
    """A table made from the frame itself: per frame the histogram of each channel, from it a 256-entry
    table by ``rule``, and the table applied.  ``rule`` "equalize" is ``cv2.equalizeHist``'s table;
    "stretch" maps the range left after clipping the fractions ``clip`` (``(lo, hi)`` or one for both, in
    ``[0, 0.5)``, kept as ``round(f * 65536)``) of the darkest and brightest pixels onto 0..255, rounding half
    up; ``clip=0`` is min-max normalisation.  ``channels`` names the channels that are levelled (``None``:
    all; the others pass unchanged); with ``link`` they share one table made from the sum of their
    histograms, which keeps the hue.  ``Level.equalize`` and ``Level.stretch`` are the two rules' builders."""
    rule: str
    rule_code: int
    mask: int
    link: bool
    clip_lo: int
    clip_hi: int
    family = "level"

    def __init__(self, rule: str, clip=0.0, channels=None, link: bool = False):
        if rule not in LEVEL_RULES:
            raise ValueError(f"Level: rule must be one of {sorted(LEVEL_RULES)}, not {rule!r}")
        lo, hi = _level_clip(clip)
        if rule == "equalize" and (lo or hi):
            raise ValueError("Level: the equalize rule takes no clip")
        if not isinstance(link, (bool, np.bool_)):
            raise ValueError(f"Level: link is a bool, not {link!r}")
        fields = {"rule": rule, "rule_code": LEVEL_RULES[rule], "mask": _level_mask(channels), "link": bool(link),
                  "clip_lo": lo, "clip_hi": hi}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @classmethod
    def equalize(cls, channels=None, link: bool = False) -> "Level":
        """``cv2.equalizeHist`` per channel (``link``: one table from the masked channels' summed histograms)."""
        return cls("equalize", 0.0, channels, link)

    @classmethod
    def stretch(cls, clip=0.0, channels=None, link: bool = False) -> "Level":
        """Auto-levels: the clipped range onto 0..255."""
        return cls("stretch", clip, channels, link)

    @property
    def min_channels(self) -> int:
        """3 when ``channels`` names channel 1 or 2 (such a filter takes 3-channel frames only), else 1."""
        return 3 if self.mask >> 1 else 1

    @property
    def args(self) -> tuple:
        return self.rule_code, self.mask, int(self.link), self.clip_lo, self.clip_hi


def _level_frame(name: str, a, level: Level) -> np.ndarray:
    a = _conv_frame(name, a)
    if level.min_channels == 3 and (a.ndim != 3 or a.shape[2] != 3):
        raise ValueError(f"{name}: the filter names channel 1 or 2; frames are H x W x 3, not shape {a.shape}")
    return a


def _level_one(name: str, src, level: Level, dst, ctx) -> np.ndarray:
    src = np.ascontiguousarray(_level_frame(name, src, level))
    dst = _rank_dst(name, src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).level_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *level.args)
    return dst


def _hist_frames(name: str, frames: Sequence) -> tuple:
    srcs = [np.ascontiguousarray(_conv_frame(name, f)) for f in frames]
    chans = {1 if s.ndim == 2 else s.shape[2] for s in srcs}
    if len(chans) > 1:
        raise ValueError(f"{name}: the frames of one call have one channel count")
    return srcs, (chans.pop() if chans else 1)


def calc_hist(src: np.ndarray, ctx: Optional[Context] = None) -> np.ndarray:
    """The histogram of a uint8 ``H x W`` or ``H x W x 3`` frame, counted on the GPU: a ``(channels, 256)`` uint32
    array, ``[c, v]`` the pixels whose channel ``c`` is ``v`` -- ``cv2.calcHist([src], [c], None, [256], [0, 256])``
    for every channel, as integers.  A frame larger than the context's staging is counted in pieces."""
    return calc_hist_frames([src], ctx)[0]


def calc_hist_frames(frames: Sequence, ctx: Optional[Context] = None) -> List:
    """``calc_hist`` of separately stored frames of one channel count and mixed sizes in one call."""
    srcs, channels = _hist_frames("calc_hist_frames", frames)
    if not srcs:
        return []
    hists = np.zeros((len(srcs), channels, 256), np.uint32)
    (ctx or get_context()).hist_frames_host(srcs, channels, hists)
    return list(hists)


def equalize_hist(src: np.ndarray, dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.equalizeHist(src)`` on uint8 ``H x W`` input, bit-exact.  On ``H x W x 3`` every channel is
    equalised by its own histogram: ``cv2.merge([cv2.equalizeHist(c) for c in cv2.split(src)])``.  ``dst`` as
    for ``lut``, and it may be ``src``."""
    return _level_one("equalize_hist", src, Level.equalize(), dst, ctx)


def auto_levels(src: np.ndarray, clip=0.0, link: bool = False, dst: Optional[np.ndarray] = None,
                ctx: Optional[Context] = None) -> np.ndarray:
    """Auto-contrast: ``Level.stretch(clip, link=link)`` on a uint8 ``H x W`` or ``H x W x 3`` frame.  ``dst`` as for
    ``lut``, and it may be ``src``."""
    return _level_one("auto_levels", src, Level.stretch(clip, None, link), dst, ctx)


def level_frames(frames: Sequence, level: Level, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Level`` over separately stored frames of one channel count and mixed sizes in one call, each frame by
    its own histogram.  Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    if not isinstance(level, Level):
        raise ValueError("level_frames: level is a Level")
    return _frames_call("level_frames", [_level_frame("level_frames", f, level) for f in frames], outs,
                        lambda *a: (ctx or get_context()).level_frames_host(*a, *level.args))


# -- CLAHE: cv2.createCLAHE(clipLimit, tileGridSize).apply ---------------------------------------------

CLAHE_MAX_TILES = 16  # an axis of the grid (csrc/vf_clahe_plan.h kMaxTilesAxis)
CLAHE_MAX_CLIP_Q8 = 1 << 24  # the clip limit in units of 1 / 256 (kMaxClipQ8)


def _clahe_clip(clip_limit) -> int:
    """``clip_limit`` -- a number whose 256-fold is an integer in ``0 .. 2**24``; 0: no clipping -- as that integer."""
    if isinstance(clip_limit, (bool, np.bool_)):
        raise ValueError(f"Clahe: clip_limit is a number, not {clip_limit!r}")
    try:
        f = float(clip_limit)
    except (TypeError, ValueError):
        raise ValueError(f"Clahe: clip_limit is a number, not {clip_limit!r}") from None
    if not 0.0 <= f <= CLAHE_MAX_CLIP_Q8 / 256:  # a NaN fails this too
        raise ValueError(f"Clahe: clip_limit = {f!r}; a clip limit is in [0, {CLAHE_MAX_CLIP_Q8 // 256}]")
    q = f * 256
    if q != int(q):
        raise ValueError(f"Clahe: clip_limit = {f!r}; clip_limit * 256 must be an integer (there is no approximate path)")
    return int(q)


def _clahe_grid(tile_grid_size) -> tuple:
    """``tile_grid_size`` -- cv2's ``(tiles_x, tiles_y)``, 1 .. 16 each."""
    try:
        tx, ty = tile_grid_size
        if any(isinstance(t, (bool, np.bool_)) or int(t) != t for t in (tx, ty)):
            raise TypeError
        tx, ty = int(tx), int(ty)
    except (TypeError, ValueError):
        raise ValueError(f"Clahe: tile_grid_size is (tiles_x, tiles_y), not {tile_grid_size!r}") from None
    if not (1 <= tx <= CLAHE_MAX_TILES and 1 <= ty <= CLAHE_MAX_TILES):
        raise ValueError(f"Clahe: tile_grid_size = {tile_grid_size!r}; 1 .. {CLAHE_MAX_TILES} tiles an axis")
    return tx, ty


def _clahe_mask(channels) -> int:
    try:
        return _level_mask(channels)
    except ValueError as e:
        raise ValueError(str(e).replace("Level:", "Clahe:", 1)) from None


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Clahe:
    """Contrast-limited adaptive histogram equalisation, ``cv2.createCLAHE(clip_limit, tile_grid_size).apply``: the
    frame, extended by reflection to whole tiles, is cut into ``tile_grid_size = (tiles_x, tiles_y)`` tiles (1 .. 16 an
    axis); every tile's histogram is clipped at ``clip_limit`` times its mean bin (0: not clipped), the excess given
    back, and made into a table; a pixel is the blend of the four nearest tiles' tables.  ``clip_limit * 256`` must
    be an integer (2.0, 2.5, 4.0 and 40.0 all are).  ``channels`` names the channels that are filtered, each on
    its own (``None``: all; the others pass unchanged); cv2 itself takes one channel."""
    clip_limit: float
    clip_q8: int
    tiles_x: int
    tiles_y: int
    mask: int
    family = "clahe"

    def __init__(self, clip_limit=40.0, tile_grid_size=(8, 8), channels=None):
        q = _clahe_clip(clip_limit)
        tx, ty = _clahe_grid(tile_grid_size)
        fields = {"clip_limit": q / 256, "clip_q8": q, "tiles_x": tx, "tiles_y": ty, "mask": _clahe_mask(channels)}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @property
    def min_channels(self) -> int:
        """3 when ``channels`` names channel 1 or 2 (such a filter takes 3-channel frames only), else 1."""
        return 3 if self.mask >> 1 else 1

    @property
    def args(self) -> tuple:
        return self.clip_q8, self.tiles_x, self.tiles_y, self.mask


def _clahe_frame(name: str, a, f: Clahe) -> np.ndarray:
    a = _conv_frame(name, a)
    if f.min_channels == 3 and (a.ndim != 3 or a.shape[2] != 3):
        raise ValueError(f"{name}: the filter names channel 1 or 2; frames are H x W x 3, not shape {a.shape}")
    return a


def clahe(src: np.ndarray, clip_limit=40.0, tile_grid_size=(8, 8), channels=None, dst: Optional[np.ndarray] = None,
          ctx: Optional[Context] = None) -> np.ndarray:
    """``cv2.createCLAHE(clip_limit, tile_grid_size).apply(src)`` on a uint8 ``H x W`` frame, bit-exact by this
    project's rule; on ``H x W x 3`` every channel of ``channels`` (``None``: all) on its own.  ``dst`` as
    for ``lut``, and it may be ``src``."""
    f = Clahe(clip_limit, tile_grid_size, channels)
    src = np.ascontiguousarray(_clahe_frame("clahe", src, f))
    dst = _rank_dst("clahe", src, dst)
    nch = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).clahe_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], nch, *f.args)
    return dst


class _ClaheObject:
    """What ``create_clahe`` returns: ``cv2.createCLAHE``'s object for 8-bit frames."""

    def __init__(self, clip_limit, tile_grid_size, ctx):
        self._filter = Clahe(clip_limit, tile_grid_size)
        self._ctx = ctx

    def apply(self, src: np.ndarray, dst: Optional[np.ndarray] = None) -> np.ndarray:
        f = self._filter
        return clahe(src, f.clip_limit, (f.tiles_x, f.tiles_y), None, dst, self._ctx)

    def getClipLimit(self) -> float:
        return self._filter.clip_limit

    def getTilesGridSize(self) -> tuple:
        return self._filter.tiles_x, self._filter.tiles_y

    def setClipLimit(self, clip_limit) -> None:
        self._filter = Clahe(clip_limit, self.getTilesGridSize())

    def setTilesGridSize(self, tile_grid_size) -> None:
        self._filter = Clahe(self._filter.clip_limit, tile_grid_size)


def create_clahe(clip_limit=40.0, tile_grid_size=(8, 8), ctx: Optional[Context] = None) -> _ClaheObject:
    """Drop-in for ``cv2.createCLAHE(clipLimit, tileGridSize)``: an object with ``apply(src)``, ``getClipLimit`` and
    ``getTilesGridSize`` (and their setters).  ``apply`` takes a uint8 ``H x W`` frame as cv2's does; an ``H x W x 3``
    frame has every channel filtered on its own."""
    return _ClaheObject(clip_limit, tile_grid_size, ctx)


def clahe_frames(frames: Sequence, f: Clahe, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Clahe`` over separately stored frames of one channel count and mixed sizes in one call.  Returns ndarrays
    (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    if not isinstance(f, Clahe):
        raise ValueError("clahe_frames: the filter is a Clahe")
    return _frames_call("clahe_frames", [_clahe_frame("clahe_frames", a, f) for a in frames], outs,
                        lambda *a: (ctx or get_context()).clahe_frames_host(*a, *f.args))


# -- the affine warp: cv2.warpAffine, cv2.flip, cv2.rotate(ROTATE_180) ----------------------------------

WARP_INTERPOLATIONS = {"linear": 0, "nearest": 1}  # the C ABI's interp
WARP_FLIPS = {"h": 1, "v": 2, "both": 3, 1: 1, 0: 2, -1: 3}  # the C ABI's mode, by name and by cv2.flip's code
INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16  # cv2's flag values, for ``warp_affine(flags=...)``
_SIZES_ARE_KEPT = "frames keep their size (resize, rotate by 90 degrees and dsize != frame size are not built)"


def invert_affine(matrix) -> tuple:
    """The map from destination to source of a forward 2 x 3 ``matrix``, by ``cv2.warpAffine``'s own formula in
    its own order on Python floats (a singular matrix gives what cv2 gives: D = 0)."""
    m0, m1, m2, m3, m4, m5 = matrix
    d = m0 * m4 - m1 * m3
    d = 1.0 / d if d != 0 else 0.0
    a11 = m4 * d
    a22 = m0 * d
    m0 = a11
    m1 *= -d
    m3 *= -d
    m4 = a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return m0, m1, b1, m3, m4, b2


def _warp_matrix(matrix) -> tuple:
    try:
        a = np.asarray(matrix, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"Warp: matrix is 2 x 3 numbers, not {matrix!r}") from None
    if a.shape != (2, 3):
        raise ValueError(f"Warp: matrix is 2 x 3, not shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError("Warp: every entry of matrix is finite")
    return tuple(float(v) for v in a.reshape(6))


def _warp_value(border_value) -> tuple:
    try:
        v = [border_value] * 3 if np.ndim(border_value) == 0 else list(border_value)
        if len(v) == 4:  # a cv2 Scalar: B, G, R and an unused fourth
            v = v[:3]
        if len(v) != 3 or any(isinstance(x, (bool, np.bool_)) or int(x) != x for x in v):
            raise TypeError
        v = tuple(int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"Warp: border_value is an integer or (B, G, R) integers, not {border_value!r}") from None
    if any(x < 0 or x > 255 for x in v):
        raise ValueError(f"Warp: border_value = {border_value!r}; a byte is in 0 .. 255")
    return v


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Warp:
    """An affine warp that keeps the frame's size, ``cv2.warpAffine(src, matrix, (W, H))`` or ``cv2.flip``:
    ``matrix`` is the 2 x 3 forward map as cv2 takes it (``inverse_map=True``: it already maps destination to source,
    cv2's ``WARP_INVERSE_MAP``), or ``flip`` is "h", "v" or "both" (or cv2.flip's 1, 0, -1) and the map is resolved for
    every frame's own size, so one value mirrors frames of mixed sizes.  ``interpolation`` "linear" or "nearest";
    ``border`` "constant" (cv2.warpAffine's default, with ``border_value`` an integer or (B, G, R)), "replicate" or
    "reflect101".  Bit-exact by the fixed-point rule of DESIGN.md 24."""
    m: Optional[tuple]  # destination to source, six floats; None for a flip
    mode: int
    interpolation: str
    interp_code: int
    border: str
    border_code: int
    value: tuple
    family = "warp"

    def __init__(self, matrix=None, flip=None, interpolation="linear", border="constant", border_value=0,
                 inverse_map=False):
        if (matrix is None) == (flip is None):
            raise ValueError("Warp: give exactly one of matrix and flip")
        if flip is not None:
            try:
                mode = None if isinstance(flip, (bool, np.bool_)) else WARP_FLIPS.get(flip)
            except TypeError:
                mode = None
            if mode is None:
                raise ValueError(f"Warp: flip is \"h\", \"v\" or \"both\" (or cv2.flip's 1, 0, -1), not {flip!r}")
            m = None
        else:
            mode = 0
            m = _warp_matrix(matrix)
            if not inverse_map:
                m = tuple(float(v) for v in invert_affine(m))
                if not all(np.isfinite(v) for v in m):
                    raise ValueError("Warp: the inverse of matrix is not finite")
        try:
            icode = WARP_INTERPOLATIONS[interpolation]
        except (KeyError, TypeError):
            raise ValueError(f"Warp: interpolation must be one of {sorted(WARP_INTERPOLATIONS)}, not {interpolation!r}") from None
        try:
            bcode = BORDERS[border]
        except (KeyError, TypeError):
            raise ValueError(f"Warp: border must be one of {sorted(BORDERS)}, not {border!r}") from None
        fields = {"m": m, "mode": mode, "interpolation": interpolation, "interp_code": icode, "border": border,
                  "border_code": bcode, "value": _warp_value(border_value)}
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    @property
    def args(self) -> tuple:
        return self.m, self.mode, self.interp_code, self.border_code, self.value


def _warp_one(name: str, src, f: Warp, dst, ctx) -> np.ndarray:
    src = np.ascontiguousarray(_conv_frame(name, src))
    dst = _rank_dst(name, src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).warp_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *f.args)
    return dst


def _warp_flags(flags, inverse_map: bool) -> tuple:
    """``flags`` -- "linear", "nearest" or cv2's integer (INTER_NEAREST 0, INTER_LINEAR 1, | WARP_INVERSE_MAP 16) -- as
    (interpolation name, inverse_map)."""
    if isinstance(flags, str):
        return flags, inverse_map
    if isinstance(flags, (bool, np.bool_)) or not isinstance(flags, (int, np.integer)) or int(flags) & ~(1 | WARP_INVERSE_MAP):
        raise ValueError(f"warp_affine: flags is \"linear\", \"nearest\" or INTER_NEAREST / INTER_LINEAR with an optional "
                         f"WARP_INVERSE_MAP, not {flags!r} (cubic, area and Lanczos are not built)")
    return ("linear" if int(flags) & 1 else "nearest"), inverse_map or bool(int(flags) & WARP_INVERSE_MAP)


def warp_affine(src: np.ndarray, M, dsize=None, flags="linear", border: str = "constant", border_value=0,
                dst: Optional[np.ndarray] = None, inverse_map: bool = False, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.warpAffine(src, M, (W, H), flags=..., borderMode=..., borderValue=...)`` on uint8 ``H x W`` or
    ``H x W x 3`` input whose size is kept: ``dsize``, when given, must be the frame's ``(W, H)``.  ``dst`` as for
    ``lut``; it may be ``src`` (the source is the staged copy)."""
    interpolation, inverse = _warp_flags(flags, inverse_map)
    f = Warp(M, None, interpolation, border, border_value, inverse)
    a = _conv_frame("warp_affine", src)
    if dsize is not None:
        try:
            same = tuple(int(v) for v in dsize) == (a.shape[1], a.shape[0]) and len(dsize) == 2
        except (TypeError, ValueError):
            same = False
        if not same:
            raise ValueError(f"warp_affine: dsize = {dsize!r} for a frame of (W, H) = ({a.shape[1]}, {a.shape[0]}); "
                             + _SIZES_ARE_KEPT)
    return _warp_one("warp_affine", src, f, dst, ctx)


def flip(src: np.ndarray, code, dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.flip(src, code)``: 0 flips around the x axis (vertically), 1 around the y axis
    (horizontally), -1 both; "v", "h" and "both" name the same."""
    if isinstance(code, (int, np.integer)) and not isinstance(code, (bool, np.bool_)):
        code = 1 if code > 0 else -1 if code < 0 else 0  # cv2: any positive, any negative
    return _warp_one("flip", src, Warp(flip=code, interpolation="nearest"), dst, ctx)


def rotate(src: np.ndarray, code, dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """``cv2.rotate(src, cv2.ROTATE_180)``: ``code`` "180" (or cv2's 1).  The 90 degree codes change the frame's shape
    and are refused."""
    if isinstance(code, (bool, np.bool_)) or code not in ("180", 1):
        raise ValueError(f"rotate: code = {code!r}; " + _SIZES_ARE_KEPT)
    return _warp_one("rotate", src, Warp(flip="both", interpolation="nearest"), dst, ctx)


def warp_frames(frames: Sequence, f: Warp, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Warp`` over separately stored frames of one channel count and mixed sizes in one call.  Returns ndarrays
    (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    if not isinstance(f, Warp):
        raise ValueError("warp_frames: the filter is a Warp")
    return _frames_call("warp_frames", [_conv_frame("warp_frames", a) for a in frames], outs,
                        lambda *a: (ctx or get_context()).warp_frames_host(*a, *f.args))


# -- the resize: cv2.resize -------------------------------------------------------------------------

RESIZE_INTERPOLATIONS = {"nearest": 0, "linear": 1, "area": 3}  # VF_INTER_*: cv2's INTER_NEAREST, INTER_LINEAR, INTER_AREA
RESIZE_MAX_SIDE = 32767


def _resize_interp(interpolation) -> int:
    if isinstance(interpolation, str) and interpolation in RESIZE_INTERPOLATIONS:
        return RESIZE_INTERPOLATIONS[interpolation]
    if isinstance(interpolation, (int, np.integer)) and not isinstance(interpolation, (bool, np.bool_)):
        if int(interpolation) in (2, 4):
            raise ValueError(f"Resize: interpolation {int(interpolation)} (cv2's INTER_CUBIC 2, INTER_LANCZOS4 4) is not "
                             "built; \"nearest\" 0, \"linear\" 1 and \"area\" 3 are")
        if int(interpolation) in RESIZE_INTERPOLATIONS.values():
            return int(interpolation)
    raise ValueError(f"Resize: interpolation must be one of {sorted(RESIZE_INTERPOLATIONS)} (or cv2's 0, 1, 3), "
                     f"not {interpolation!r}")


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Resize:
    """``cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=...)`` on uint8 frames of 1 or 3 channels: ``dsize`` is
    ``(width, height)``, or it is ``None`` (or ``(0, 0)``) and ``fx``, ``fy`` scale every frame's own size to
    ``rint(W fx) x rint(H fy)``, half to even, so one value resizes frames of mixed sizes.  ``interpolation``
    "nearest", "linear" or "area" (or cv2's 0, 1, 3); area is built for integer shrink factors of 1 to 16 (another
    scale is refused for the frame that has it), and linear at exactly 2 x 2 runs as area, as in cv2.  The first
    filter value whose result has another size than its operand: ``out_size(w, h)`` says which.  Bit-exact by
    the rule of DESIGN.md 26."""
    dsize: Optional[tuple]  # (width, height); None: by fx, fy
    fx: float
    fy: float
    interpolation: str
    interp_code: int
    family = "resize"

    def __init__(self, dsize=None, fx=0, fy=0, interpolation="linear"):
        code = _resize_interp(interpolation)
        if dsize is not None:
            try:
                d = tuple(dsize)
                ok = len(d) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in d)
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f"Resize: dsize is (width, height) integers or None, not {dsize!r}")
            d = (int(d[0]), int(d[1]))
            if d == (0, 0):
                d = None  # cv2's empty Size(): by fx, fy
            elif not all(1 <= v <= RESIZE_MAX_SIDE for v in d):
                raise ValueError(f"Resize: dsize = {dsize!r}; a side is 1 to {RESIZE_MAX_SIDE}")
            dsize = d
        try:
            fx, fy = float(fx), float(fy)
        except (TypeError, ValueError):
            raise ValueError(f"Resize: fx and fy are numbers, not {fx!r}, {fy!r}") from None
        if dsize is None and not (np.isfinite(fx) and np.isfinite(fy) and fx > 0 and fy > 0):
            raise ValueError(f"Resize: without dsize, fx and fy are finite and positive, not {fx!r}, {fy!r}")
        name = {v: k for k, v in RESIZE_INTERPOLATIONS.items()}[code]
        for k, v in (("dsize", dsize), ("fx", fx), ("fy", fy), ("interpolation", name), ("interp_code", code)):
            object.__setattr__(self, k, v)

    @property
    def args(self) -> tuple:
        """``(dw, dh, fx, fy, interp)``: the C arguments, and a VF_STEP_RESIZE step's data."""
        dw, dh = self.dsize if self.dsize is not None else (0, 0)
        return dw, dh, self.fx, self.fy, self.interp_code

    def out_size(self, w: int, h: int) -> tuple:
        """``(width, height)`` of the result for a frame of ``w`` x ``h`` (vf_resize_plan.h's out_size)."""
        w, h = int(w), int(h)
        if not (1 <= w <= RESIZE_MAX_SIDE and 1 <= h <= RESIZE_MAX_SIDE):
            raise ValueError(f"Resize: a frame of {w} x {h}; a side is 1 to {RESIZE_MAX_SIDE}")
        if self.dsize is not None:
            return self.dsize
        out = tuple(int(min(max(np.rint(np.float64(n) * np.float64(f)), -2.0 ** 31), 2.0 ** 31 - 1)) for n, f in ((w, self.fx), (h, self.fy)))
        if min(out) < 1:
            raise ValueError(f"Resize: a frame of {w} x {h} resizes to {out[0]} x {out[1]}: a side of 0")
        if max(out) > RESIZE_MAX_SIDE:
            raise ValueError(f"Resize: a frame of {w} x {h} resizes to {out[0]} x {out[1]}; a side is at most {RESIZE_MAX_SIDE}")
        return out


def _sized_dst(name: str, src: np.ndarray, size: tuple, dst) -> np.ndarray:
    """``dst`` made or checked for a result of ``size`` = (width, height) and ``src``'s channels."""
    shape = (size[1], size[0]) + src.shape[2:]
    if dst is None:
        return np.empty(shape, np.uint8)
    if not isinstance(dst, np.ndarray) or dst.shape != shape or dst.dtype != np.uint8 or not dst.flags.c_contiguous:
        raise ValueError(f"{name}: dst must be a C-contiguous uint8 array of the result's shape {shape}, not "
                         f"{getattr(dst, 'shape', type(dst).__name__)}")
    return dst


def _sized_frames_call(name: str, srcs: List[np.ndarray], outs: Optional[List], out_size, call) -> List:
    """``_frames_call`` where frame i's result has ``out_size(width, height)``."""
    srcs = [np.ascontiguousarray(s) for s in srcs]
    chans = {1 if s.ndim == 2 else s.shape[2] for s in srcs}
    if len(chans) > 1:
        raise ValueError(f"{name}: the frames of one call have one channel count")
    if outs is not None and len(outs) != len(srcs):
        raise ValueError(f"{name}: outs must hold one array a frame")
    outs = [(np.empty_like(s) if outs is None else o) if not s.size
            else _sized_dst(name, s, out_size(s.shape[1], s.shape[0]), None if outs is None else o)
            for s, o in zip(srcs, outs if outs is not None else [None] * len(srcs))]
    live = [(s, o) for s, o in zip(srcs, outs) if s.size]
    if live:
        call([s for s, _ in live], [o for _, o in live], [s.shape[1] for s, _ in live],
             [s.shape[0] for s, _ in live], chans.pop())
    return outs


def resize(src: np.ndarray, dsize=None, fx=0, fy=0, interpolation="linear", dst: Optional[np.ndarray] = None,
           ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=...)`` on uint8 ``H x W`` or ``H x W x 3``
    input (``Resize`` has the arguments).  ``dst``, when given, has the result's shape; it may not share memory with
    ``src`` unless the two sizes are equal."""
    f = Resize(dsize, fx, fy, interpolation)
    src = np.ascontiguousarray(_conv_frame("resize", src))
    if not src.size:
        return _rank_dst("resize", src, dst)
    dst = _sized_dst("resize", src, f.out_size(src.shape[1], src.shape[0]), dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    (ctx or get_context()).resize_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *f.args)
    return dst


def resize_frames(frames: Sequence, f: Resize, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Resize`` over separately stored frames of one channel count and mixed sizes in one call.  Returns ndarrays
    (or fills ``outs``, C-contiguous arrays of the results' shapes)."""
    if not isinstance(f, Resize):
        raise ValueError("resize_frames: the filter is a Resize")
    return _sized_frames_call("resize_frames", [_conv_frame("resize_frames", a) for a in frames], outs, f.out_size,
                              lambda *a: (ctx or get_context()).resize_frames_host(*a, *f.args))


# -- filter chains: a program of filters between one upload and one download ----------------------

STEP_TABLE, STEP_CONV, STEP_RANK, STEP_BINARY = 0, 1, 2, 3  # VF_STEP_* (include/vfilter.h)
STEP_MIX = 5  # VF_STEP_MIX: 4 names no kind and stays refused
STEP_SEP = 7  # VF_STEP_SEP: 6 stays refused as well
STEP_LEVEL = 8  # VF_STEP_LEVEL: 9 stays refused as well
STEP_CLAHE = 10  # VF_STEP_CLAHE: 11 stays refused as well
STEP_WARP = 12  # VF_STEP_WARP: 13 stays refused as well
STEP_RESIZE = 14  # VF_STEP_RESIZE: 15 stays refused as well
BINARY_OPS = {"subtract": 0, "add": 1, "absdiff": 2, "min": 3, "max": 4}  # VF_BIN_*
CHAIN_MAX_STEPS = 8  # VF_CHAIN_MAX_STEPS
MORPH_OPS = ("erode", "dilate", "open", "close", "gradient", "tophat", "blackhat")

_INVERT_TABLE = bytes(255 - v for v in range(256))


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Combine:
    """A two-input step of a ``Chain``: ``op(a, b)`` per byte, ``op`` one of "subtract"
    (``max(a - b, 0)``), "add" (``min(a + b, 255)``), "absdiff", "min", "max" -- ``cv2.subtract``,
    ``cv2.add``, ``cv2.absdiff``, ``cv2.min``, ``cv2.max`` on uint8.  ``a`` and ``b`` are each a filter
    value (``Invert``, ``Table``, ``Kernel``, ``Rank``, ``Mix``, ``Separable``, ``Level``, ``Clahe``, ``Warp``, another ``Combine``), a ``Chain``, or ``None``
    for the value entering the ``Combine``; both are applied to that value."""
    op: str
    op_code: int
    a: object
    b: object

    def __init__(self, op: str, a=None, b=None):
        if op not in BINARY_OPS:
            raise ValueError(f"combine: op must be one of {sorted(BINARY_OPS)}, not {op!r}")
        for name, v in (("a", a), ("b", b)):
            if v is not None and not isinstance(v, _CHAIN_ITEMS + (Chain, Combine)):  # another Combine nests
                raise ValueError(f"combine: {name} is a filter value, a Chain or None, not {type(v).__name__}")
        for name, v in (("op", op), ("op_code", BINARY_OPS[op]), ("a", a), ("b", b)):
            object.__setattr__(self, name, v)


def _unary_step(f, a: int) -> tuple:
    """The program step of one single-filter value reading value ``a``."""
    if isinstance(f, Invert):
        return (STEP_TABLE, a, 0, 0, _INVERT_TABLE, 0, 0)
    if isinstance(f, Table):
        return (STEP_TABLE, a, 0, 0, f.planar, 0, 0)
    if isinstance(f, Kernel):
        return (STEP_CONV, a, 0, 0, f.weights, f.shift, f.border_code)
    if isinstance(f, Rank):
        return (STEP_RANK, a, 0, f.op_code, f.element, 0, f.border_code)
    if isinstance(f, Mix):
        return (STEP_MIX, a, 0, f.rounding_code, f.matrix, f.shift, 0)
    if isinstance(f, Separable):
        return (STEP_SEP, a, 0, f.rounding_code, (f.kx, f.ky, f.divisor), f.shift, f.border_code)
    if isinstance(f, Level):
        return (STEP_LEVEL, a, 0, f.rule_code, (f.mask, int(f.link), f.clip_lo, f.clip_hi), 0, 0)
    if isinstance(f, Clahe):
        return (STEP_CLAHE, a, 0, 0, (f.mask, f.clip_q8, f.tiles_x, f.tiles_y), 0, 0)
    if isinstance(f, Warp):
        return (STEP_WARP, a, 0, 0, (f.m if f.m is not None else (0.0,) * 6, f.mode, f.interp_code, f.value), 0, f.border_code)
    if isinstance(f, Resize):
        return (STEP_RESIZE, a, 0, 0, f.args, 0, 0)
    # existing callers match the list up to "not <type>" word for word, so a newer filter value is named after it
    raise ValueError("chain: a step is Invert, Table, Kernel, Rank, Mix, Separable, Level, Combine or Chain, or a Clahe, "
                     f"not {type(f).__name__} (a Warp is a step as well)")


def _check_program(steps: Sequence[tuple]) -> None:
    """The structure of a program (csrc/vf_chain_plan.h validate), as ``ValueError``s."""
    n = len(steps)
    if n < 1:
        raise ValueError("chain: an empty program")
    if n > CHAIN_MAX_STEPS:
        raise ValueError(f"chain: a program of {n} steps; at most {CHAIN_MAX_STEPS} (VF_CHAIN_MAX_STEPS)")
    read = [False] * (n + 1)
    for i, st in enumerate(steps, 1):
        kind, a, b = st[0], st[1], st[2]
        for name, v in (("a", a),) + ((("b", b),) if kind == STEP_BINARY else ()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"chain: step {i}: operand {name} = {v!r} is not a value")
            if v >= i:
                raise ValueError(f"chain: step {i}: operand {name} = {v} is not an earlier value "
                                 f"(a step reads values 0..{i - 1}; no forward reference)")
            read[v] = True
    for v in range(n):
        if not read[v]:
            raise ValueError(f"chain: value {v} is read by no step (a dead value)")


@dataclasses.dataclass(frozen=True, init=False, eq=False)
class Chain:
    """A program of filters run on the GPU between one upload and one download (raw frames) or one
    decode and one encode (JPEG): exactly what running its steps one after the other on whole frames
    gives, every step with whole-frame borders.

    ``Chain(steps)``: each of ``steps`` -- ``Invert``, ``Table``, ``Kernel``, ``Rank``, ``Mix``, ``Separable``,
    ``Level``, ``Clahe``, ``Warp``, ``Combine`` or a nested ``Chain``, which is flattened -- is applied to the result of the one
    before.  A chain with a ``Level``, a ``Clahe`` or a ``Warp`` reads whole frames: a frame larger than the context's staging is
    refused, not cut into bands.
    ``Chain.program(entries)`` takes the program itself: value 0 is the frame, value i the result of
    entry i (1-based); an entry is ``(filter value, a)`` or ``(binary op name, a, b)`` with ``a`` and
    ``b`` earlier values.  At most 8 steps; every value but the last is read.  A bad program raises
    ``ValueError`` here, before a GPU context exists."""
    steps: tuple  # (kind, a, b, op, data, shift, border) per step; data: table bytes, weights, element, None
    family = "chain"

    def __init__(self, steps):
        if isinstance(steps, _CHAIN_ITEMS + (Chain, Combine)):
            steps = [steps]
        prog: List[tuple] = []
        out = _lower(list(steps), 0, prog)
        if out != len(prog):  # e.g. Chain([]): nothing to run
            raise ValueError("chain: an empty program")
        _check_program(prog)
        object.__setattr__(self, "steps", tuple(prog))

    @classmethod
    def program(cls, entries) -> "Chain":
        prog = []
        for i, e in enumerate(entries, 1):
            if not isinstance(e, (tuple, list)) or len(e) not in (2, 3):
                raise ValueError(f"chain: entry {i} is (filter value, a) or (binary op, a, b)")
            if len(e) == 3:
                if e[0] not in BINARY_OPS:
                    raise ValueError(f"chain: entry {i}: op must be one of {sorted(BINARY_OPS)}, not {e[0]!r}")
                prog.append((STEP_BINARY, e[1], e[2], BINARY_OPS[e[0]], None, 0, 0))
            else:
                prog.append(_unary_step(e[0], e[1]))
        _check_program(prog)
        self = object.__new__(cls)
        object.__setattr__(self, "steps", tuple(prog))
        return self

    @property
    def args(self) -> tuple:
        return (self.steps,)

    @property
    def table_channels(self) -> int:
        """3 when a step is a 3-channel table (such a chain takes 3-channel frames only), else 1."""
        return 3 if any(st[0] == STEP_TABLE and len(st[4]) == 768 for st in self.steps) else 1

    @property
    def has_mix(self) -> bool:
        """True when a step is a colour matrix (such a chain takes 3-channel frames only)."""
        return any(st[0] == STEP_MIX for st in self.steps)

    @property
    def level_channels(self) -> int:
        """3 when a level step names channel 1 or 2 (such a chain takes 3-channel frames only), else 1."""
        return 3 if any(st[0] in (STEP_LEVEL, STEP_CLAHE) and st[4][0] >> 1 for st in self.steps) else 1

    @property
    def has_resize(self) -> bool:
        """True when a step is a ``Resize``: the result's size is ``out_size``'s, not the frame's."""
        return any(st[0] == STEP_RESIZE for st in self.steps)

    def out_size(self, w: int, h: int) -> tuple:
        """``(width, height)`` of the result for a frame of ``w`` x ``h``: a ``Resize`` step makes a value of another
        size, every other step one of its operand's.  ``ValueError`` for a two-input step whose operands differ in
        size, naming the step.  Pure Python on purpose: ``chain`` and ``chain_frames`` allocate results with it
        before a GPU context exists, and a ``Chain`` is built and sized on machines without one;
        ``Context.chain_out_size`` is the library's own answer (csrc/vf_chain_plan.h ``value_sizes``), and the GPU
        tests hold the two equal, refusals included."""
        sizes = [(int(w), int(h))]
        for i, (kind, a, b, _op, data, _shift, _border) in enumerate(self.steps, 1):
            size = sizes[a]
            if kind == STEP_RESIZE:
                dw, dh, fx, fy, interp = data
                size = Resize((dw, dh) if dw or dh else None, fx, fy, interp).out_size(*size)
            elif kind == STEP_BINARY and sizes[b] != size:
                raise ValueError(f"chain: step {i}: operand a (value {a}) is {size[0]} x {size[1]} and operand b (value {b}) "
                                 f"is {sizes[b][0]} x {sizes[b][1]}: a binary step's operands have one size")
            sizes.append(size)
        return sizes[-1]

    def __len__(self) -> int:
        return len(self.steps)


_CHAIN_ITEMS = (Invert, Table, Kernel, Rank, Mix, Separable, Level, Clahe, Warp, Resize)


def _lower(item, cur: int, prog: List[tuple]) -> int:
    """Append the steps of ``item`` applied to value ``cur``; returns the value that holds the result."""
    if item is None:
        return cur
    if isinstance(item, (list, tuple)):
        for it in item:
            cur = _lower(it, cur, prog)
        return cur
    if isinstance(item, Chain):  # its program, moved: its value 0 is cur, its value i is base + i
        base = len(prog)
        for (kind, a, b, op, data, shift, border) in item.steps:
            prog.append((kind, base + a if a else cur, (base + b if b else cur) if kind == STEP_BINARY else 0, op, data,
                         shift, border))
        return len(prog)
    if isinstance(item, Combine):
        va = _lower(item.a, cur, prog)
        vb = _lower(item.b, cur, prog)
        prog.append((STEP_BINARY, va, vb, item.op_code, None, 0, 0))
        return len(prog)
    prog.append(_unary_step(item, cur))
    return len(prog)


def Morph(op: str, element=None, iterations: int = 1, border: str = "constant") -> Chain:
    """``cv2.morphologyEx(src, op, element, iterations=iterations)`` as a ``Chain``.  With E^n / D^n
    for n successive erosions / dilations by ``element``: "erode" E^n, "dilate" D^n, "open" D^n(E^n x),
    "close" E^n(D^n x), "gradient" subtract(D^n x, E^n x), "tophat" subtract(x, open),
    "blackhat" subtract(close, x).  ``iterations`` is limited by the chain's 8 steps."""
    if op not in MORPH_OPS:
        raise ValueError(f"morphology_ex: op must be one of {list(MORPH_OPS)}, not {op!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"morphology_ex: iterations must be a positive integer, not {iterations!r}")
    n = int(iterations)
    need = {"erode": n, "dilate": n, "open": 2 * n, "close": 2 * n}.get(op, 2 * n + 1)
    if need > CHAIN_MAX_STEPS:
        raise ValueError(f"morphology_ex: {op} with iterations={n} is a chain of {need} steps; a chain has at most "
                         f"{CHAIN_MAX_STEPS} (VF_CHAIN_MAX_STEPS), so iterations is limited by that cap")
    e, d = [Rank.erode(element, border)] * n, [Rank.dilate(element, border)] * n
    if op == "erode":
        return Chain(e)
    if op == "dilate":
        return Chain(d)
    if op == "open":
        return Chain(e + d)
    if op == "close":
        return Chain(d + e)
    if op == "gradient":
        return Chain([Combine("subtract", Chain(d), Chain(e))])
    if op == "tophat":
        return Chain([Combine("subtract", None, Chain(e + d))])
    return Chain([Combine("subtract", Chain(d + e), None)])


def _as_chain(c) -> Chain:
    return c if isinstance(c, Chain) else Chain(c)


def _chain_frame(name: str, a, c: Chain) -> np.ndarray:
    a = _conv_frame(name, a)
    if c.table_channels == 3 and (a.ndim != 3 or a.shape[2] != 3):
        raise ValueError(f"{name}: the chain has a 3-channel table; frames are H x W x 3, not shape {a.shape}")
    if c.has_mix and (a.ndim != 3 or a.shape[2] != 3):
        raise ValueError(f"{name}: the chain has a colour matrix; frames are H x W x 3, not shape {a.shape}")
    if c.level_channels == 3 and (a.ndim != 3 or a.shape[2] != 3):
        raise ValueError(f"{name}: a level or CLAHE step names channel 1 or 2; frames are H x W x 3, not shape {a.shape}")
    return a


def chain(src: np.ndarray, steps, dst: Optional[np.ndarray] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """Run a ``Chain`` (or a list of steps, as for ``Chain``) on a uint8 ``H x W`` or ``H x W x 3`` frame
    with one upload and one download.  ``dst`` as for ``filter2d``, and it may be ``src``."""
    c = _as_chain(steps)
    src = np.ascontiguousarray(_chain_frame("chain", src, c))
    if c.has_resize and src.size:  # the result has Chain.out_size's size; a dst of another shape is refused
        dst = _sized_dst("chain", src, c.out_size(src.shape[1], src.shape[0]), dst)
    else:
        dst = _rank_dst("chain", src, dst)
    channels = 1 if src.ndim == 2 else src.shape[2]
    if src.size:
        (ctx or get_context()).chain_frames_host([src], [dst], [src.shape[1]], [src.shape[0]], channels, *c.args)
    return dst


def chain_frames(frames: Sequence, chain, outs: Optional[List] = None, ctx: Optional[Context] = None) -> List:
    """A ``Chain`` over separately stored frames of one channel count and mixed sizes in one call.
    Returns ndarrays (or fills ``outs``, C-contiguous arrays of the frames' shapes)."""
    c = _as_chain(chain)
    if c.has_resize:
        return _sized_frames_call("chain_frames", [_chain_frame("chain_frames", f, c) for f in frames], outs, c.out_size,
                                  lambda *a: (ctx or get_context()).chain_frames_host(*a, *c.args))
    return _frames_call("chain_frames", [_chain_frame("chain_frames", f, c) for f in frames], outs,
                        lambda *a: (ctx or get_context()).chain_frames_host(*a, *c.args))


def morphology_ex(src: np.ndarray, op: str, element=None, iterations: int = 1, dst: Optional[np.ndarray] = None,
                  border: str = "constant", ctx: Optional[Context] = None) -> np.ndarray:
    """Drop-in for ``cv2.morphologyEx(src, op, element, iterations=iterations)`` on uint8 ``H x W`` or
    ``H x W x 3`` input, ``op`` one of "erode", "dilate", "open", "close", "gradient", "tophat",
    "blackhat" (``Morph`` has the programs).  Equal to cv2 for the default border, "constant"."""
    return chain(src, Morph(op, element, iterations, border), dst, ctx)


def invert_frames(frames: Sequence, outs: Optional[List] = None,
                  ctx: Optional[Context] = None) -> List:
    """Invert separately stored frames (ndarrays or bytes-likes; mixed sizes allowed) with
    one gathered pipeline pass.  Returns ndarrays (or fills ``outs``)."""
    srcs = [np.ascontiguousarray(f) if isinstance(f, np.ndarray) else np.frombuffer(f, dtype=np.uint8)
            for f in frames]
    if outs is None:
        outs = [np.empty_like(s) for s in srcs]
    (ctx or get_context()).invert_frames_host(srcs, outs, [s.nbytes for s in srcs])
    return outs
