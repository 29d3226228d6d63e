"""LutWorker: the reference's filter plugin with another filter in it.

The reference's plugin is ``decode -> cv2.bitwise_not -> encode`` (inverter.py:29-46).  A user
who swaps line 41 for any other per-pixel filter -- gamma, brightness / contrast, levels,
threshold, posterize, solarize, per-channel colour curves -- has a 256-entry table, i.e.
``cv2.LUT(frame, table)``.  ``LutWorker`` is ``InverterWorker`` with that table in place of the
inversion and the same plugin contract, ``__call__(frame_bytes) -> bytes``:

  JPEG mode   ``InverterWorker``'s, with ``filters.Table`` as the worker's filter: the fused GPU pass
              of ``TurboJPEG.filter_*`` (decode -> table -> encode, no host round trip of the
              pixels) for ``__call__``, ``process_batch``, ``submit_batch`` and ``submit_ring_batch``.
  raw mode    ``vf_lut_frames_host`` (upload, kernel, download) for ``__call__`` and
              ``process_batch``; batches are not queued asynchronously (``inverter.FilterWorker``:
              ``submit_batch`` runs them at once, as ``delay > 0`` does for the inverter).

``table`` is as for ``vfilter.lut``; with three channels, channel c is channel c of the BGR frame
(inverter.py:32 decodes to BGR), and a raw frame is interleaved 3-channel bytes from channel 0.
"""
from __future__ import annotations

import argparse

import numpy as np

from .filters import Table
from .inverter import FilterWorker, worker_main


class LutWorker(FilterWorker):
    def __init__(self, *args, table, **kw):
        filt = Table(table)  # refuses a bad table before any GPU work
        self.table = np.array(table, dtype=np.uint8)
        super().__init__(*args, filter=filt, **kw)
        if self.verbose:
            print(f"LUT worker: {filt.channels}-channel table")

    def raw_batch(self, srcs, metas, dsts) -> None:
        self.ctx.lut_frames_host(srcs, dsts, [s.nbytes for s in srcs], self.filter.planar, self.filter.channels)


def main(argv=None):
    """The inverter worker's command line plus ``--table-npy``."""
    ap = argparse.ArgumentParser(description="256-entry table (cv2.LUT) worker for video processing (MI355X backend)")
    ap.add_argument("--table-npy", required=True, metavar="PATH",
                    help="numpy file with the uint8 table: 256 entries, or (256, 3) for one table per BGR channel")

    def own(args) -> dict:
        table = np.load(args.table_npy, allow_pickle=False)
        Table(table)  # a bad table ends here, before a GPU context exists
        return {"table": table}

    worker_main(ap, argv, "LUT worker", LutWorker, own)


if __name__ == "__main__":
    main()
