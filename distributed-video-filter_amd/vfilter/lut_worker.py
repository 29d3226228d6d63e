"""LutWorker: the reference's filter plugin with another filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user
who swaps line 41 for any other per-pixel filter -- gamma, brightness / contrast, levels,
threshold, posterize, solarize, per-channel colour curves -- has a 256-entry table, i.e.
``cv2.LUT(frame, table)``.  ``LutWorker`` is ``InverterWorker`` with that table in place of the
inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   the fused GPU pass of ``TurboJPEG.lut*`` (decode -> table -> encode, no host round
              trip of the pixels) for ``__call__``, ``process_batch``, ``submit_batch`` and
              ``submit_ring_batch``; tickets are collected by ``InverterWorker.poll_batch``.
  raw mode    ``vf_lut_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches are not queued asynchronously (``submit_batch`` runs
              them at once, as ``delay > 0`` does for the inverter).

``table`` is as for ``vfilter.lut``; with three channels, channel c is channel c of the BGR frame
(inverter.py:32 decodes to BGR), and a raw frame is interleaved 3-channel bytes from channel 0.
"""
from __future__ import annotations

import argparse
import time
from typing import List, Sequence

import numpy as np

from . import wire
from .filters import as_table
from .inverter import InverterWorker, pin_to_gpu_node
from .worker import Worker, WorkerFailed


class LutWorker(InverterWorker):
    def __init__(self, *args, table, **kw):
        self.table_planar, self.table_channels = as_table(table)  # refuses a bad table before any GPU work
        self.table = np.array(table, dtype=np.uint8)
        super().__init__(*args, **kw)
        if self.verbose:
            print(f"LUT worker: {self.table_channels}-channel table")

    # -- one frame --------------------------------------------------------------------------
    def __call__(self, frame_bytes):
        if self.delay > 0:                                          # inverter.py:37-38
            time.sleep(self.delay)
        if self.jpeg:
            return self.jpeg.lut(frame_bytes, self.table)           # inverter.py:32 -> LUT -> :44, fused
        frame = np.frombuffer(frame_bytes, dtype=np.uint8)          # inverter.py:34, any size
        out = np.empty_like(frame)
        self.ctx.lut_frames_host([frame], [out], [frame.nbytes], self.table_planar, self.table_channels)
        return out

    # -- a dispatched batch -----------------------------------------------------------------
    def process_batch(self, frames: Sequence, metas: Sequence[wire.FrameMeta], outs: Sequence) -> List:
        if self.delay > 0:
            time.sleep(self.delay * len(frames))
        if self.jpeg:
            try:
                return self.jpeg.lut_batch(list(frames), self.table)
            except Exception:  # retry frame by frame so a bad frame fails alone (worker.py:74-76)
                return self._frame_by_frame(frames, metas, outs)
        srcs, dsts = [], []
        for f, o in zip(frames, outs):
            src = f if isinstance(f, np.ndarray) else np.frombuffer(f, dtype=np.uint8)
            srcs.append(src)
            dsts.append(o if o is not None else np.empty(src.nbytes, np.uint8))
        try:
            self.ctx.lut_frames_host(srcs, dsts, [s.nbytes for s in srcs], self.table_planar, self.table_channels)
        except Exception:  # e.g. a frame that is not whole pixels: it fails alone
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
                return ("jpeg", self.jpeg.lut_batch_submit(list(frames), self.table), list(frames), list(outs))
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
            t = self.jpeg.lut_batch_submit_addrs(ina, nbs, self.table)
        except Exception:  # a frame the host parser refuses: the per-frame views path
            return None
        return ("jpeg_ring", t, ina + np.uint64(sb), sb, ring, cols)


def main(argv=None):
    """The inverter worker's command line plus ``--table-npy``."""
    ap = argparse.ArgumentParser(description="256-entry table (cv2.LUT) worker for video processing (MI355X backend)")
    ap.add_argument("--table-npy", required=True, metavar="PATH",
                    help="numpy file with the uint8 table: 256 entries, or (256, 3) for one table per BGR channel")
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
    table = np.load(args.table_npy, allow_pickle=False)
    as_table(table)  # a bad table ends here, before a GPU context exists
    pin_to_gpu_node(args.device)
    worker = LutWorker(args.host, args.distribute_port, args.collect_port, args.delay, use_jpeg=not args.raw,
                       table=table, device=args.device, batch=args.batch, inflight=args.inflight,
                       protocol=args.protocol, transport=args.transport, verbose=args.verbose)
    try:
        worker.start()
    except WorkerFailed as e:
        print(f"LUT worker: giving up: {e}")
        raise SystemExit(3)
    finally:
        worker.close()


if __name__ == "__main__":
    main()
