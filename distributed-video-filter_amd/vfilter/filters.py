"""The filter entry points: ``cv2.bitwise_not`` semantics on the MI355X.

Reference call site: ``inverted = cv2.bitwise_not(frame)`` (inverter.py:41), frame a
C-contiguous uint8 H x W x 3 ndarray (a read-only view from ``np.frombuffer`` on the raw
path, inverter.py:34).  ``bitwise_not`` keeps that signature: a new same-shape, same-dtype
array comes back and the input is never written.  The work runs in libvfilter_hip.so;
there is no CPU fallback.
"""
from __future__ import annotations

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
