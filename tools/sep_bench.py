#!/usr/bin/env python3
"""Time of the separable-filter kernel next to the convolution and the 3-channel table kernels, same
buffers, same process (profiles/sep_raw_bench.txt, profiles/sep_jpeg_bench.txt).

    tools/sep_bench.py raw   [--frames 32] [--launches 20] [--rounds 7]
    tools/sep_bench.py probe [--frames 32]     # one launch per variant, for rocprofv3 --pmc
    tools/sep_bench.py jpeg  [--frames 32] [--iters 10] [--rounds 7]

raw    1080p x 32 frames in device memory, random content, as one frame of 1920 x 34560 x 3.
       Variants: lut3 (vf_lut_device with three tables: the yardstick), vf_conv_device with gaussian7
       under both settings of VF_CONV_FORM, and vf_sep_device with binomial7 (the same filter in 14
       taps), fixed-point Gaussians of 15 and 31 taps, and boxes of 3, 15 and 31 -- each with the
       vertical sums the launcher picks and with VF_SEP_FORM=wide (32-bit sums; the same kernel where
       the taps do not fit 16 bits), and the 31-tap ones under every tile height VF_SEP_ROWS allows.
       A measurement is `launches` back-to-back launches on the null stream between two device
       synchronises, host clock; a round takes every variant once, in turn; median, min and max over
       the rounds after one warm-up round.
jpeg   vf_jpeg_bench_sep (box 5, a 31-tap Gaussian) against vf_jpeg_bench_conv (gaussian3) and
       vf_jpeg_bench_invert with VF_JPEG_FUSE=0 -- the same pixel round trip -- alternating.
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


def _set(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def _variants(ctx, frames):
    import numpy as np
    import vfilter
    from vfilter import Separable
    from vfilter import kernels as K
    w, h = 1920, 1080 * frames
    n = w * h * 3
    d_src, d_out = ctx.alloc_device(n), ctx.alloc_device(n)
    ctx.upload(d_src, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), n)
    ctx.sync()
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    g7, s7 = vfilter.as_kernel(K.gaussian7())

    def conv(form):
        def launch():
            _set("VF_CONV_FORM", form)
            ctx.conv_device(d_src, d_out, w, h, 3, g7, s7, 0)
        return launch

    def sep(s, form=None, rows=None):
        def launch():
            _set("VF_SEP_FORM", form)
            _set("VF_SEP_ROWS", rows)
            ctx.sep_device(d_src, d_out, w, h, 3, *s.args)
        return launch

    seps = {"binomial7": Separable(K.binomial_taps(7)), "gauss15": Separable.gaussian(15, 2.5),
            "gauss31": Separable.gaussian(31, 5.0), "box3": Separable.box(3), "box15": Separable.box(15),
            "box31": Separable.box(31)}
    variants = {"lut3": lambda: ctx.lut_device(d_src, d_out, n, t3, c3),
                "conv_gaussian7/wide": conv("wide"), "conv_gaussian7/narrow": conv("narrow")}
    for name, s in seps.items():
        variants[f"sep_{name}"] = sep(s)
        variants[f"sep_{name}/wide"] = sep(s, "wide")
    for name in ("gauss31", "box31"):
        for rows in ("16", "24"):
            variants[f"sep_{name}/rows{rows}"] = sep(seps[name], None, rows)
    for rows in ("16", "24", "32"):
        variants[f"sep_binomial7/rows{rows}"] = sep(seps["binomial7"], None, rows)
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
    conv_best = min(out["variants"][k]["us"]["median"] for k in out["variants"] if k.startswith("conv_"))
    b7 = out["variants"]["sep_binomial7"]["us"]
    out["sep7_vs_conv7"] = {"conv_best_us": conv_best, "sep_us": b7["median"], "sep_spread_us": b7["max"] - b7["min"],
                            "sep_below_conv_by_more_than_the_spread": conv_best - b7["median"] > b7["max"] - b7["min"]}
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
    from vfilter import Separable
    from vfilter import kernels as K
    scenes = [J.synthetic_scene(s, 1080, 1920) for s in range(min(args.frames, 8))]
    jpgs = [J.encode(scenes[i % len(scenes)], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(args.frames)]
    g3, s3 = vfilter.as_kernel(K.gaussian3())
    box5, g31 = Separable.box(5), Separable.gaussian(31, 5.0)
    which = ["invert", "invert_unfused", "conv_gaussian3", "sep_box5", "sep_gauss31"]
    res = {w: [] for w in which}
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=args.frames) as ctx:
        def run(w, iters):
            if w == "conv_gaussian3":
                return ctx.jpeg_bench_conv(jpgs, g3, s3, 0, 85, J.TJSAMP_422, 0, iters=iters)[0]
            if w == "sep_box5":
                return ctx.jpeg_bench_sep(jpgs, *box5.args, 85, J.TJSAMP_422, 0, iters=iters)[0]
            if w == "sep_gauss31":
                return ctx.jpeg_bench_sep(jpgs, *g31.args, 85, J.TJSAMP_422, 0, iters=iters)[0]
            if w == "invert":
                return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
            os.environ["VF_JPEG_FUSE"] = "0"  # invert_unfused: the pixel round trip (read per call)
            try:
                return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
            finally:
                del os.environ["VF_JPEG_FUSE"]
        for rnd in range(args.rounds + 1):
            for w in which:
                ms = run(w, 2 if rnd == 0 else args.iters)
                if rnd:
                    res[w].append(ms)
    return {"mode": "jpeg", "frames": args.frames, "iters": args.iters, "rounds": args.rounds,
            "variants": {w: {"batch_ms": stats(r), "batch_ms_runs": r} for w, r in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "probe", "jpeg"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"raw": raw, "probe": probe, "jpeg": jpeg}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
