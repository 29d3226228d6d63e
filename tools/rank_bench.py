#!/usr/bin/env python3
"""Kernel-only time of the rank filters next to the table and the convolution kernel, HBM-resident,
same buffers, same process (profiles/rank_raw_bench.txt, profiles/rank_jpeg_bench.txt).

    tools/rank_bench.py raw   [--frames 32] [--launches 100] [--rounds 7]
    tools/rank_bench.py jpeg  [--frames 32] [--iters 20] [--rounds 5] [--which median3,erode5,invert_unfused]
    tools/rank_bench.py probe [--frames 32]          # one launch per variant, to run under rocprofv3 --pmc;
                                                     # tools/conv_bench.py pmc CSV ... summarises the counters

raw    1080p x 32 frames in device memory, random content, filtered as ONE 1920 x (1080 * frames)
       x 3 image, so a launch covers the same bytes as the table kernel's one launch.  Variants:
       erode by rect3, rect5, rect7 and cross3, median3 and median5; as yardsticks vf_lut_device
       (lut3, memory-bound at 2 bytes of traffic per output byte) and the convolution of the same
       side (conv3, conv5, conv7: the narrow form, sum|K| <= 128).  A measurement is `launches`
       back-to-back launches on the null stream between two device synchronises, host clock; a
       round takes every variant once, in turn; the figures are the median, min and max over the
       rounds after one warm-up round.
jpeg   vf_jpeg_bench_rank against vf_jpeg_bench_invert with VF_JPEG_FUSE=0 -- the same pixel round
       trip without a filter -- on one batch of 1080p scene frames (q85, 4:2:2), alternating.  With
       VFILTER_LIB pointing at another build's library only the variants that library has can run
       (the parent commit's: --which invert_unfused).
No GPU, no number: every path here needs the device.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distributed-video-filter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _ranks():
    from vfilter import Rank, elements
    return {"rect3": Rank.erode(elements.rect(3)), "rect5": Rank.erode(elements.rect(5)),
            "rect7": Rank.erode(elements.rect(7)), "cross3": Rank.erode(elements.cross(3)),
            "median3": Rank.median(3), "median5": Rank.median(5)}


def _variants(ctx, frames):
    import numpy as np
    import vfilter
    from vfilter import kernels as K
    w, h = 1920, 1080 * frames
    n = w * h * 3
    d_src, d_out = ctx.alloc_device(n), ctx.alloc_device(n)
    ctx.upload(d_src, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), n)
    ctx.sync()
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    k5 = np.random.default_rng(3).integers(-5, 6, (5, 5))
    k7 = np.random.default_rng(4).integers(-2, 3, (7, 7))
    convs = {"conv3": vfilter.as_kernel(K.gaussian3()), "conv5": vfilter.as_kernel((k5, 2)),
             "conv7": vfilter.as_kernel((k7, 1))}
    variants = {"lut3": lambda: ctx.lut_device(d_src, d_out, n, t3, c3)}
    for name, (wts, s) in convs.items():
        assert abs(wts.astype(int)).sum() <= 128  # the narrow form holds them
        variants[name] = lambda wts=wts, s=s: ctx.conv_device(d_src, d_out, w, h, 3, wts, s, 0)
    for name, r in _ranks().items():
        variants[name] = lambda r=r: ctx.rank_device(d_src, d_out, w, h, 3, *r.args)
    return variants, n, (d_src, d_out)


def raw(args):
    import vfilter
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        variants, n, bufs = _variants(ctx, args.frames)
        us = {k: [] for k in variants}
        for rnd in range(args.rounds + 1):
            for name, launch in variants.items():
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(args.launches):
                    launch()
                ctx.sync()
                if rnd:  # round 0 warms up every variant
                    us[name].append((time.perf_counter() - t0) / args.launches * 1e6)
        for d in bufs:
            ctx.free_device(d)
    out = {"mode": "raw", "bytes": n, "launches": args.launches, "rounds": args.rounds, "variants": {}}
    base = statistics.median(us["lut3"])
    for name, xs in us.items():
        s = stats(xs)
        out["variants"][name] = {"us": s, "GBps_out": {k: n / v / 1e3 for k, v in s.items()},
                                 "time_vs_lut3": s["median"] / base}
    return out


def probe(args):
    """Each variant once (after one untimed warm-up launch each), for a counters-only profiler run."""
    import vfilter
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        variants, n, bufs = _variants(ctx, args.frames)
        for _ in range(2):
            for launch in variants.values():
                launch()
                ctx.sync()
        for d in bufs:
            ctx.free_device(d)
    return {"mode": "probe", "bytes": n, "variants": list(variants)}


def jpeg(args):
    import vfilter
    from oracle import jpeg as J
    scenes = [J.synthetic_scene(s, 1080, 1920) for s in range(min(args.frames, 8))]
    jpgs = [J.encode(scenes[i % len(scenes)], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(args.frames)]
    which = args.which.split(",")
    res = {w: [] for w in which}
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=args.frames) as ctx:
        def run(w, iters):
            if w == "invert":
                return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
            if w == "invert_unfused":  # the pixel round trip (VF_JPEG_FUSE is read per call)
                os.environ["VF_JPEG_FUSE"] = "0"
                try:
                    return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
                finally:
                    del os.environ["VF_JPEG_FUSE"]
            from vfilter import Rank, elements
            ranks = {"median3": Rank.median(3), "median5": Rank.median(5), "erode3": Rank.erode(elements.rect(3)),
                     "erode5": Rank.erode(elements.rect(5)), "erode7": Rank.erode(elements.rect(7))}
            return ctx.jpeg_bench_rank(jpgs, *ranks[w].args, 85, J.TJSAMP_422, 0, iters=iters)[0]
        for rnd in range(args.rounds + 1):
            for w in which:
                ms = run(w, 2 if rnd == 0 else args.iters)
                if rnd:
                    res[w].append(ms)
    return {"mode": "jpeg", "frames": args.frames, "iters": args.iters, "rounds": args.rounds,
            "lib": os.environ.get("VFILTER_LIB", "in-tree"),
            "variants": {w: {"batch_ms": stats(r), "batch_ms_runs": r} for w, r in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "jpeg", "probe"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--which", default="median3,median5,erode3,erode5,erode7,invert_unfused",
                    help="jpeg: median3 | median5 | erode3 | erode5 | erode7 (rect) | invert_unfused (VF_JPEG_FUSE=0) | invert")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 7 if args.mode == "raw" else 5
    out = {"raw": raw, "jpeg": jpeg, "probe": probe}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
