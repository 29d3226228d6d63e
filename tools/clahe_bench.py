#!/usr/bin/env python3
"""Time of CLAHE next to the 3-channel table kernel and the level filter, same buffers, same process
(profiles/clahe_raw_bench.txt, profiles/clahe_jpeg_bench.txt).

    tools/clahe_bench.py raw  [--frames 32] [--calls 10] [--rounds 5]
    tools/clahe_bench.py jpeg [--iters 10] [--rounds 5]

raw    1080p x 32 BGR frames resident in device memory, with three contents: random bytes, a constant
       frame, and synthetic scenes (vfilter.synthetic).  A call filters the 32 frames one after the other
       on the null stream, each frame with its own launches, as the JPEG path and the host path do.
       Variants per content: lut3 (vf_lut_device with three tables), level (vf_level_device, equalize:
       memset, histogram, apply), clahe8 and clahe16 (vf_clahe_device, limit 2.0, grids 8 x 8 and 16 x 16:
       memset, tile histograms, tables, blend).  The kernels' settings -- VF_CLAHE_REPLICAS,
       VF_CLAHE_HIST_WGS, VF_CLAHE_APPLY_WGS -- are read once by the library, so each setting is a run of
       this tool with the variable set; the settings of a run are in its output.  A measurement is
       `calls` back-to-back calls between two device synchronises, host clock; a round takes every
       variant once, in turn; median, min and max over the rounds after one warm-up round.  The result
       reports CLAHE as a ratio to lut3 and to level, and constant over random.
jpeg   vf_jpeg_bench_clahe (limit 2.0, 8 x 8) against vf_jpeg_bench_invert, _lut and _level (equalize) at
       512 x 512 x 64 and 1080p x 32, alternating.
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

SETTINGS = ("VF_CLAHE_REPLICAS", "VF_CLAHE_HIST_WGS", "VF_CLAHE_APPLY_WGS")


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def raw(args):
    import numpy as np
    import vfilter
    from vfilter.synthetic import synthetic_frame
    w, h = 1920, 1080
    one = w * h * 3
    n = one * args.frames
    scenes = np.concatenate([synthetic_frame(s, 1080, 1920) for s in range(4)])
    contents = {"random": np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8),
                "constant": np.full(n, 128, np.uint8),
                "scene": np.tile(scenes.reshape(-1), (args.frames + 3) // 4)[:n]}
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    out = {"mode": "raw", "bytes": n, "frames": args.frames, "calls": args.calls, "rounds": args.rounds,
           "settings": {k: os.environ.get(k, "") for k in SETTINGS}, "contents": {}}
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        d_src, d_out = ctx.alloc_device(n), ctx.alloc_device(n)

        def per_frame(fn):
            def call():
                for f in range(args.frames):
                    fn(d_src + f * one, d_out + f * one)
            return call

        variants = {"lut3": per_frame(lambda s, d: ctx.lut_device(s, d, one, t3, c3)),
                    "level": per_frame(lambda s, d: ctx.level_device(s, d, w, h, 3, 0)),
                    "clahe8": per_frame(lambda s, d: ctx.clahe_device(s, d, w, h, 3, 512, 8, 8, 0)),
                    "clahe16": per_frame(lambda s, d: ctx.clahe_device(s, d, w, h, 3, 512, 16, 16, 0))}
        for cname, data in contents.items():
            ctx.upload(d_src, data, n)
            ctx.sync()
            us = {k: [] for k in variants}
            for rnd in range(args.rounds + 1):
                for name, call in variants.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        call()
                    ctx.sync()
                    if rnd:  # round 0 warms up every variant
                        us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
            res = {}
            for name, xs in us.items():
                s = stats(xs)
                res[name] = {"us": s, "us_per_frame": s["median"] / args.frames, "GBps_read": n / s["median"] / 1e3}
            for k in ("clahe8", "clahe16"):
                res[k + "_vs_lut3"] = res[k]["us"]["median"] / res["lut3"]["us"]["median"]
                res[k + "_vs_level"] = res[k]["us"]["median"] / res["level"]["us"]["median"]
            out["contents"][cname] = res
        for d in (d_src, d_out):
            ctx.free_device(d)
    c = out["contents"]
    for k in ("clahe8", "clahe16", "level"):
        out[k + "_constant_over_random"] = c["constant"][k]["us"]["median"] / c["random"][k]["us"]["median"]
    return out


def jpeg(args):
    import numpy as np
    import vfilter
    from oracle import jpeg as J
    perm = np.random.default_rng(2).permutation(256).astype(np.uint8)
    which = ["invert", "lut", "level_equalize", "clahe"]
    out = {"mode": "jpeg", "iters": args.iters, "rounds": args.rounds,
           "settings": {k: os.environ.get(k, "") for k in SETTINGS}, "shapes": {}}
    for name, (hh, ww, count) in {"512x512x64": (512, 512, 64), "1080px32": (1080, 1920, 32)}.items():
        scenes = [J.synthetic_scene(s, hh, ww) for s in range(4)]
        jpgs = [J.encode(scenes[i % 4], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(count)]
        res = {w: [] for w in which}
        with vfilter.Context(0, max_frame_bytes=ww * hh * 3, max_batch=count) as ctx:
            def run(w, iters):
                if w == "invert":
                    return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
                if w == "lut":
                    return ctx.jpeg_bench_lut(jpgs, perm, 1, 85, J.TJSAMP_422, 0, iters=iters)[0]
                if w == "level_equalize":
                    return ctx.jpeg_bench_level(jpgs, 0, 0, 0, 0, 0, 85, J.TJSAMP_422, 0, iters=iters)[0]
                return ctx.jpeg_bench_clahe(jpgs, 512, 8, 8, 0, 85, J.TJSAMP_422, 0, iters=iters)[0]
            for rnd in range(args.rounds + 1):
                for w in which:
                    ms = run(w, 2 if rnd == 0 else args.iters)
                    if rnd:
                        res[w].append(ms)
        out["shapes"][name] = {w: {"batch_ms": stats(r), "batch_ms_runs": r} for w, r in res.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "jpeg"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"raw": raw, "jpeg": jpeg}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
