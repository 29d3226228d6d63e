"""ConvWorker: the reference's filter plugin with a neighbourhood filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user who
swaps line 41 for a blur, a Gaussian, a sharpening or an edge filter has one call,
``cv2.filter2D(frame, -1, kernel)``.  ``ConvWorker`` is ``InverterWorker`` with that call in place
of the inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   the GPU pass of ``TurboJPEG.filter2d*`` (decode -> filter2D -> encode, no host round
              trip of the pixels) for ``__call__``, ``process_batch``, ``submit_batch`` and
              ``submit_ring_batch``; tickets are collected by ``InverterWorker.poll_batch``.
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
import time
from typing import List, Sequence

import numpy as np

from . import wire
from .filters import as_kernel, border_code
from .inverter import InverterWorker, pin_to_gpu_node
from .worker import Worker, WorkerFailed

DEFAULT_SHAPE = (480, 480, 3)  # inverter.py:34


def _shape3(shape) -> tuple:
    s = tuple(int(v) for v in shape)
    if len(s) == 2:
        s = s + (1,)
    if len(s) != 3 or s[2] not in (1, 3) or s[0] <= 0 or s[1] <= 0:
        raise ValueError(f"a raw frame is H x W or H x W x 3, not shape {tuple(shape)}")
    return s


class ConvWorker(InverterWorker):
    def __init__(self, *args, kernel, border: str = "reflect101", shape=DEFAULT_SHAPE, **kw):
        self.weights, self.shift = as_kernel(kernel)  # refuses a bad kernel before any GPU work
        self.border = border
        self.border_code = border_code(border)
        self.shape = _shape3(shape)
        super().__init__(*args, **kw)
        if self.verbose:
            print(f"filter2D worker: {self.weights.shape[0]} x {self.weights.shape[1]} kernel / 2^{self.shift}, {border}")

    @property
    def kernel(self):
        return self.weights, self.shift

    def _frame_shape(self, nbytes: int, meta=None) -> tuple:
        shape = _shape3(meta.shape) if meta is not None and getattr(meta, "shape", None) else self.shape
        if shape[0] * shape[1] * shape[2] != nbytes:
            raise ValueError(f"cannot reshape a raw frame of {nbytes} bytes into shape {shape}")  # inverter.py:34
        return shape

    def _raw(self, srcs: List[np.ndarray], shapes: List[tuple], dsts: List[np.ndarray]) -> None:
        chans = {s[2] for s in shapes}
        if len(chans) != 1:
            raise ValueError("the frames of one batch have one channel count")
        self.ctx.conv_frames_host(srcs, dsts, [s[1] for s in shapes], [s[0] for s in shapes], chans.pop(),
                                  self.weights, self.shift, self.border_code)

    # -- one frame --------------------------------------------------------------------------
    def __call__(self, frame_bytes):
        if self.delay > 0:                                          # inverter.py:37-38
            time.sleep(self.delay)
        if self.jpeg:                                               # inverter.py:32 -> filter2D -> :44
            return self.jpeg.filter2d(frame_bytes, self.kernel, self.border)
        frame = np.frombuffer(frame_bytes, dtype=np.uint8)          # inverter.py:34
        out = np.empty_like(frame)
        self._raw([frame], [self._frame_shape(frame.nbytes)], [out])
        return out

    # -- a dispatched batch -----------------------------------------------------------------
    def process_batch(self, frames: Sequence, metas: Sequence[wire.FrameMeta], outs: Sequence) -> List:
        if self.delay > 0:
            time.sleep(self.delay * len(frames))
        if self.jpeg:
            try:
                return self.jpeg.filter2d_batch(list(frames), self.kernel, self.border)
            except Exception:  # retry frame by frame so a bad frame fails alone (worker.py:74-76)
                return self._frame_by_frame(frames, metas, outs)
        try:
            srcs, dsts, shapes = [], [], []
            for f, m, o in zip(frames, metas, outs):
                src = f if isinstance(f, np.ndarray) else np.frombuffer(f, dtype=np.uint8)
                shapes.append(self._frame_shape(src.nbytes, m))
                srcs.append(src)
                dsts.append(o if o is not None else np.empty(src.nbytes, np.uint8))
            self._raw(srcs, shapes, dsts)
        except Exception:  # e.g. a frame of another size: it fails alone
            return self._frame_by_frame(frames, metas, outs)
        return dsts

    def _frame_by_frame(self, frames, metas, outs) -> List:
        delay, self.delay = self.delay, 0.0  # already slept for the batch
        try:
            return Worker.process_batch(self, frames, metas, outs)
        finally:
            self.delay = delay

    # -- asynchronous submission ------------------------------------------------------------
    def submit_batch(self, frames: Sequence, metas: Sequence[wire.FrameMeta], outs: Sequence):
        if self.jpeg:
            self._note_jpeg_bytes(float(sum(len(f) for f in frames)), len(frames))
        if self.jpeg and self.delay <= 0:
            try:  # staged and queued now; the loop receives the next batch while this one runs
                t = self.jpeg.filter2d_batch_submit(list(frames), self.kernel, self.border)
                return ("jpeg", t, list(frames), list(outs))
            except Exception:  # a frame the host parser refuses: frame by frame (worker.py:74-76)
                return ("done", self._frame_by_frame(frames, metas, outs), [])
        return Worker.submit_batch(self, frames, metas, outs)  # synchronous: process_batch now

    def submit_ring_batch(self, ring, cols):
        if self.delay > 0 or not self.jpeg:
            return None  # the per-frame views path: submit_batch
        sb = ring.slot_bytes
        slots, nbs = cols["slot"], cols["nbytes"]
        if len(slots) and (int(slots.min()) < 0 or int(slots.max()) >= ring.nslots or int(nbs.min()) < 0
                           or int(nbs.max()) > sb):
            return None  # a record outside this ring slice: never a raw GPU address
        ina = np.uint64(ring.base_address) + slots.astype(np.uint64) * np.uint64(2 * sb)
        self._note_jpeg_bytes(float(nbs.sum()), len(nbs))
        try:
            t = self.jpeg.filter2d_batch_submit_addrs(ina, nbs, self.kernel, self.border)
        except Exception:  # a frame the host parser refuses: the per-frame views path
            return None
        return ("jpeg_ring", t, ina + np.uint64(sb), sb, ring, cols)


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
    ap.add_argument("--distribute-port", type=int, default=5555)
    ap.add_argument("--collect-port", type=int, default=5556)
    ap.add_argument("--delay", type=float, default=0.0, help="Artificial processing delay in seconds (default: 0.0)")
    ap.add_argument("--host", default="localhost")
    ap.add_argument("--raw", action="store_true", help="raw H x W x 3 frames (use_jpeg=False); default JPEG frames")
    ap.add_argument("--device", type=int, default=None, help="GPU ordinal (default: VF_DEVICE / LOCAL_RANK / 0)")
    ap.add_argument("--batch", type=int, default=0, help="frames per request (see vfilter.inverter)")
    ap.add_argument("--inflight", type=int, default=None, help="batches in progress at once")
    ap.add_argument("--protocol", choices=("v0", "v1"), default="v1")
    ap.add_argument("--transport", choices=("auto", "zmq", "tcp"), default="auto")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    kernel = np.load(args.kernel_npy, allow_pickle=False)
    if args.shift is not None:
        kernel = (kernel, args.shift)
    as_kernel(kernel)  # a bad kernel ends here, before a GPU context exists
    _shape3(args.shape)
    pin_to_gpu_node(args.device)
    worker = ConvWorker(args.host, args.distribute_port, args.collect_port, args.delay, use_jpeg=not args.raw,
                        kernel=kernel, border=args.border, shape=args.shape, device=args.device, batch=args.batch,
                        inflight=args.inflight, protocol=args.protocol, transport=args.transport, verbose=args.verbose)
    try:
        worker.start()
    except WorkerFailed as e:
        print(f"filter2D worker: giving up: {e}")
        raise SystemExit(3)
    finally:
        worker.close()


if __name__ == "__main__":
    main()
