#!/usr/bin/env python3
"""Time of the histogram kernel and of the whole level filter next to the invert and the 3-channel table
kernels, same buffers, same process (profiles/level_raw_bench.txt, profiles/level_jpeg_bench.txt;
DESIGN.md 22.4).

    tools/level_bench.py raw  [--frames 32] [--launches 20] [--rounds 7]
    tools/level_bench.py jpeg [--iters 10] [--rounds 5]

raw    1080p x 32 BGR frames in device memory as one range of 1920 x 34560 x 3, with three contents:
       random bytes, a constant frame, and synthetic scenes (vfilter.synthetic).  Variants per content:
       invert (vf_invert_device: the stream kernel's read + write rate on the same bytes), lut3
       (vf_lut_device with three tables), hist (vf_hist_device: a memset of 3 KiB and the kernel) and
       level (vf_level_device, equalize: memset, histogram, apply).  The histogram kernel's variants --
       VF_HIST_REPLICAS, VF_HIST_NT, VF_HIST_BLOCKS -- are read once by the library, so each setting is
       a run of this tool with the variable set; the settings of a run are in its output.  A
       measurement is `launches` back-to-back calls on the null stream between two device synchronises,
       host clock; a round takes every variant once, in turn; median, min and max over the rounds after
       one warm-up round.  The result reports the constant-to-random ratio of the histogram: the cost of
       same-address conflicts.
jpeg   vf_jpeg_bench_level (equalize, stretch) against vf_jpeg_bench_lut and vf_jpeg_bench_invert at
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


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def raw(args):
    import numpy as np
    import vfilter
    from vfilter.synthetic import synthetic_frame
    w, h = 1920, 1080 * args.frames
    n = w * h * 3
    scenes = np.concatenate([synthetic_frame(s, 1080, 1920) for s in range(4)])
    contents = {"random": np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8),
                "constant": np.full(n, 128, np.uint8),
                "scene": np.tile(scenes.reshape(-1), (args.frames + 3) // 4)[:n]}
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    out = {"mode": "raw", "bytes": n, "launches": args.launches, "rounds": args.rounds,
           "settings": {k: os.environ.get(k, "") for k in ("VF_HIST_REPLICAS", "VF_HIST_NT", "VF_HIST_BLOCKS")},
           "contents": {}}
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        d_src, d_out, d_hist = ctx.alloc_device(n), ctx.alloc_device(n), ctx.alloc_device(4096)
        variants = {"invert": lambda: ctx.invert_device(d_src, d_out, n),
                    "lut3": lambda: ctx.lut_device(d_src, d_out, n, t3, c3),
                    "hist": lambda: ctx.hist_device(d_src, n, 3, d_hist),
                    "level": lambda: ctx.level_device(d_src, d_out, w, h, 3, 0)}
        for cname, data in contents.items():
            ctx.upload(d_src, data, n)
            ctx.sync()
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
            res = {}
            for name, xs in us.items():
                s = stats(xs)
                res[name] = {"us": s, "GBps_read": n / s["median"] / 1e3}
            res["hist_vs_invert"] = res["hist"]["us"]["median"] / res["invert"]["us"]["median"]
            res["level_vs_lut3"] = res["level"]["us"]["median"] / res["lut3"]["us"]["median"]
            out["contents"][cname] = res
        for d in (d_src, d_out, d_hist):
            ctx.free_device(d)
    c = out["contents"]
    out["hist_constant_over_random"] = c["constant"]["hist"]["us"]["median"] / c["random"]["hist"]["us"]["median"]
    return out


def jpeg(args):
    import numpy as np
    import vfilter
    from oracle import jpeg as J
    perm = np.random.default_rng(2).permutation(256).astype(np.uint8)
    which = ["invert", "lut", "level_equalize", "level_stretch"]
    out = {"mode": "jpeg", "iters": args.iters, "rounds": args.rounds, "shapes": {}}
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
                rule, clip = (0, 0) if w == "level_equalize" else (1, 655)
                return ctx.jpeg_bench_level(jpgs, rule, 0, 0, clip, clip, 85, J.TJSAMP_422, 0, iters=iters)[0]
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
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
