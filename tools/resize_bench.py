#!/usr/bin/env python3
"""Time of the resize next to the 3-channel table kernel and the affine warp with the equal zoom, same process
(profiles/resize_raw_bench.txt).

    tools/resize_bench.py [--frames 32] [--calls 10] [--rounds 5] [--out FILE]

Every case has a 1080p BGR result, 32 of them, from 32 resident source frames of synthetic scenes
(vfilter.synthetic, tiled to the source's size): from 3840 x 2160 (0.5 x) in linear -- which runs as area 2 x 2 --
area and nearest; from 7680 x 4320 (0.25 x) in area; from 960 x 540 (2 x) in linear and nearest; from 1920 x 1080 (1 x)
in linear.  A call filters the
32 frames one after the other on the null stream, a frame a launch, as the host path does.  The yardsticks, on
1080p frames: lut3 (vf_lut_device with three tables), and vf_warp_device in linear interpolation with the zoom
maps that read the source at the same 0.5 x and 2 x steps, whose result is 1080p as well.  The kernel's settings --
VF_RESIZE_LDS, the staged source box's budget in bytes (0: never staged), and VF_RESIZE_HROWS, the h rows' budget
(0: per pixel) -- are read by the library at every launch, so one run takes the four combinations of each linear
and nearest case.  Beside each figure: the bytes a frame moves (source read once, result written once) and what
they take at 6.3 TB/s, the HBM rate a kernel reaches on this GPU.  A measurement is `calls` back-to-back calls
between two device synchronises, host clock; a round takes every variant once, in turn; median, min and max over
the rounds after one warm-up round.  No GPU, no number.
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

LDS, HROWS = 16384, 16384  # csrc/vf_resize.hip kStageLds, and the h-row budget the sweep switches on (committed: 0)
HBM = 6.3e12               # bytes a second


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import vfilter
    from vfilter import Resize, Warp, warps
    from vfilter.synthetic import synthetic_frame
    ow, oh = 1920, 1080
    out_one = ow * oh * 3
    scene = synthetic_frame(0, 1080, 1920)
    sources = {"8k": (7680, 4320), "4k": (3840, 2160), "1080p": (1920, 1080), "540p": (960, 540)}
    cases = [("0.25x area", "8k", "area"), ("0.5x linear", "4k", "linear"), ("0.5x area", "4k", "area"), ("0.5x nearest", "4k", "nearest"),
             ("2x linear", "540p", "linear"), ("2x nearest", "540p", "nearest"), ("1x linear", "1080p", "linear")]
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    centre = ((ow - 1) / 2, (oh - 1) / 2)
    zooms = {"warp zoom 0.5 (reads at 2 x steps)": Warp(warps.zoom(0.5, centre)),
             "warp zoom 2 (reads at 0.5 x steps)": Warp(warps.zoom(2.0, centre))}
    out = {"frames": args.frames, "calls": args.calls, "rounds": args.rounds, "committed": {"lds": LDS, "hrows": 0},
           "yardsticks": {}, "cases": {}}
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        d_out = ctx.alloc_device(out_one * args.frames)
        d_src = {}
        for name, (w, h) in sources.items():
            img = np.ascontiguousarray(np.tile(scene, ((h + 1079) // 1080, (w + 1919) // 1920, 1))[:h, :w])
            d_src[name] = ctx.alloc_device(img.nbytes * args.frames)
            for f in range(args.frames):
                ctx.upload(d_src[name] + f * img.nbytes, np.roll(img, 7 * f, axis=1), img.nbytes)
        ctx.sync()

        def per_frame(fn, src, env=None):
            w, h = sources[src]
            one = w * h * 3

            def call():
                for k, v in (env or {}).items():
                    os.environ[k] = str(v)
                for f in range(args.frames):
                    fn(d_src[src] + f * one, d_out + f * out_one, w, h)
            return call

        variants = {("lut3",): per_frame(lambda s, d, w, h: ctx.lut_device(s, d, out_one, t3, c3), "1080p")}
        for name, f in zooms.items():
            variants[(name,)] = per_frame(lambda s, d, w, h, f=f: ctx.warp_device(s, d, w, h, 3, *f.args), "1080p")
        for name, src, interp in cases:
            f = Resize((ow, oh), interpolation=interp)
            settings = [(LDS, 0)] if interp == "area" or name == "0.5x linear" else \
                [(LDS, 0), (0, 0)] if interp == "nearest" else [(LDS, HROWS), (LDS, 0), (0, HROWS), (0, 0)]
            for lds, hrows in settings:
                variants[(name, src, lds, hrows)] = per_frame(lambda s, d, w, h, f=f: ctx.resize_device(s, d, w, h, 3, *f.args), src,
                                                              {"VF_RESIZE_LDS": lds, "VF_RESIZE_HROWS": hrows, "VF_RESIZE_AREA_WIDE": 1})
            if interp == "area":  # the byte kernel beside the wide-load one
                variants[(name + ", byte loads", src, LDS, 0)] = per_frame(
                    lambda s, d, w, h, f=f: ctx.resize_device(s, d, w, h, 3, *f.args), src,
                    {"VF_RESIZE_LDS": LDS, "VF_RESIZE_HROWS": 0, "VF_RESIZE_AREA_WIDE": 0})
        us = {k: [] for k in variants}
        for rnd in range(args.rounds + 1):
            for key, call in variants.items():
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                ctx.sync()
                if rnd:  # round 0 warms up every variant
                    us[key].append((time.perf_counter() - t0) / args.calls * 1e6)
        for d in [d_out] + list(d_src.values()):
            ctx.free_device(d)
    for k in ("VF_RESIZE_LDS", "VF_RESIZE_HROWS", "VF_RESIZE_AREA_WIDE"):
        os.environ.pop(k, None)
    lines = ["us a frame (a 1080p BGR result), median [min .. max] of %d rounds of %d calls over %d frames" %
             (args.rounds, args.calls, args.frames)]
    for key, xs in us.items():
        s = {k: v / args.frames for k, v in stats(xs).items()}
        src = key[1] if len(key) > 1 else "1080p"
        moved = sources[src][0] * sources[src][1] * 3 + out_one
        rec = {"us_per_frame": s, "bytes_per_frame": moved, "hbm_us": moved / HBM * 1e6}
        label = key[0] if len(key) == 1 else f"{key[0]} lds={key[2]} hrows={key[3]}"
        (out["yardsticks"] if len(key) == 1 else out["cases"])[label] = rec
        lines.append("%-44s %7.2f [%7.2f .. %7.2f]   %5.1f MB moved, %5.2f us at 6.3 TB/s" %
                     (label, s["median"], s["min"], s["max"], moved / 1e6, rec["hbm_us"]))
    print(json.dumps(out))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(out) + "\n")
        with open(args.out + ".table", "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
