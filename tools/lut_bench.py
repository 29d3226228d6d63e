#!/usr/bin/env python3
"""Kernel-only rate of the table filter next to the invert kernel, HBM-resident, same buffers,
same process (profiles/lut_raw_bench.txt, profiles/lut_jpeg_bench.txt).

    tools/lut_bench.py raw  [--frames 32] [--launches 1000] [--rounds 7] [--layout 0|1]
    tools/lut_bench.py jpeg [--frames 32] [--iters 20] [--rounds 5] [--which invert,lut3,curves3,lut1]

raw   1080p x 32 bytes in device memory, random and flat content.  A measurement is `launches`
      back-to-back launches on the null stream between two device synchronises, host clock; a
      round takes every variant once, in turn, so slow drifts hit all of them; the figures are
      the median, min and max over the rounds after one warm-up round.  GB/s counts the bytes
      filtered (input bytes; the kernel moves twice that).  --layout sets VF_LUT_LAYOUT.
jpeg  vf_jpeg_bench_lut against vf_jpeg_bench_invert on one batch of 1080p scene frames (q85,
      4:2:2): whole-batch ms and the colour stage, median / min / max over the rounds.
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


def raw(args):
    if args.layout is not None:
        os.environ["VF_LUT_LAYOUT"] = str(args.layout)
    import numpy as np
    import vfilter
    from vfilter import tables
    n = 1920 * 1080 * 3 * args.frames
    rng = np.random.default_rng(0)
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t1, c1 = vfilter.as_table(perm(1))
    t3, c3 = vfilter.as_table(tables.stack(perm(2), perm(3), perm(4)))
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        d_rand, d_flat, d_out = ctx.alloc_device(n), ctx.alloc_device(n), ctx.alloc_device(n)
        ctx.upload(d_rand, rng.integers(0, 256, n, dtype=np.uint8), n)
        ctx.memset_device(d_flat, 0x5A, n)
        ctx.sync()
        variants = {}
        for content, src in (("random", d_rand), ("flat", d_flat)):
            variants[f"invert/{content}"] = lambda src=src: ctx.invert_device(src, d_out, n)
            variants[f"lut1/{content}"] = lambda src=src: ctx.lut_device(src, d_out, n, t1, c1)
            variants[f"lut3/{content}"] = lambda src=src: ctx.lut_device(src, d_out, n, t3, c3)
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
        for d in (d_rand, d_flat, d_out):
            ctx.free_device(d)
    out = {"mode": "raw", "bytes": n, "launches": args.launches, "rounds": args.rounds,
           "layout": int(os.environ.get("VF_LUT_LAYOUT", "0") or 0), "variants": {}}
    for name, xs in us.items():
        s = stats(xs)
        base = statistics.median(us["invert/" + name.split("/")[1]])
        out["variants"][name] = {"us": s, "GBps": {k: n / v / 1e3 for k, v in s.items()},
                                 "rate_vs_invert": base / s["median"]}
    return out


def jpeg(args):
    import numpy as np
    import vfilter
    from oracle import jpeg as J
    from vfilter import tables
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(tables.stack(perm(2), perm(3), perm(4)))
    t1, c1 = vfilter.as_table(tables.gamma(2.2))
    # lut3 is three random permutations: the colour stage's worst case for LDS banks, but its
    # output is noise, which the ENCODER then pays for; curves3 is three smooth per-channel curves,
    # what a colour-grading user runs, and leaves the encoder the content it had
    s3, cs3 = vfilter.as_table(tables.stack(tables.gamma(2.2), tables.levels(1.2, -10), tables.gamma(0.8)))
    scenes = [J.synthetic_scene(s, 1080, 1920) for s in range(min(args.frames, 8))]
    jpgs = [J.encode(scenes[i % len(scenes)], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(args.frames)]
    which = args.which.split(",")
    res = {w: {"ms": [], "colour_ms": []} for w in which}
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=args.frames) as ctx:
        def run(w, iters):
            if w == "invert":
                ms, st = ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)
                return ms, st["color_invert"]
            t, c = {"lut3": (t3, c3), "curves3": (s3, cs3)}.get(w, (t1, c1))
            ms, st = ctx.jpeg_bench_lut(jpgs, t, c, 85, J.TJSAMP_422, 0, iters=iters)
            return ms, st["color_lut"]
        for rnd in range(args.rounds + 1):
            for w in which:
                ms, col = run(w, 2 if rnd == 0 else args.iters)
                if rnd:
                    res[w]["ms"].append(ms)
                    res[w]["colour_ms"].append(col)
    return {"mode": "jpeg", "frames": args.frames, "iters": args.iters, "rounds": args.rounds,
            "lib": os.environ.get("VFILTER_LIB", "in-tree"),
            "variants": {w: {"batch_ms": stats(r["ms"]), "colour_ms": stats(r["colour_ms"]),
                             "batch_ms_runs": r["ms"], "colour_ms_runs": r["colour_ms"]} for w, r in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "jpeg"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layout", type=int, default=None, choices=(0, 1))
    ap.add_argument("--which", default="invert,lut3,curves3,lut1",
                    help="jpeg: invert | lut3 (permutations) | curves3 (smooth 3-channel) | lut1 (gamma, 1 channel)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 7 if args.mode == "raw" else 5
    out = raw(args) if args.mode == "raw" else jpeg(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
