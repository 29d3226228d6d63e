#!/usr/bin/env python3
"""Time of the affine warp next to the 3-channel table kernel and the 3 x 3 convolution, same buffers, same
process (profiles/warp_raw_bench.txt).

    tools/warp_bench.py [--frames 32] [--calls 10] [--rounds 5] [--lds 0 8192 16384 32768 61440] [--rows 8 16 32] [--cross]

1080p x 32 BGR frames of synthetic scenes (vfilter.synthetic) resident in device memory.  A call filters the 32
frames one after the other on the null stream, a frame a launch, as the JPEG path and the host path do.  The
yardsticks are lut3 (vf_lut_device with three tables) and filter2d (vf_conv_device, a 3 x 3 Gaussian).  The maps
(destination to source): a horizontal flip (nearest), and in linear interpolation a half-pixel shift, a 5 degree
rotation at scale 1.1 about the centre, a 30 degree rotation and a 0.5 x shrink.  The kernel's settings --
VF_WARP_LDS, the LDS budget of the staged source box in bytes, 0 forcing the general path everywhere, and
VF_WARP_ROWS, the rows of an output tile -- are read by the library at every launch, so one run sweeps them: every
budget of --lds at the committed rows, then every tile height of --rows at the committed budget (--cross: every
budget at every height).  A measurement is
`calls` back-to-back calls between two device synchronises, host clock; a round takes every variant once, in
turn; median, min and max over the rounds after one warm-up round.  No GPU, no number.
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

LDS, ROWS = 16384, 16  # csrc/vf_warp.hip kWarpLds, kTileRows


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lds", type=int, nargs="*", default=[0, 8192, 16384, 32768, 61440])
    ap.add_argument("--rows", type=int, nargs="*", default=[8, 16, 32])
    ap.add_argument("--cross", action="store_true", help="every budget of --lds at every tile height of --rows")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import vfilter
    from vfilter import Warp, warps
    from vfilter.synthetic import synthetic_frame
    w, h = 1920, 1080
    one = w * h * 3
    n = one * args.frames
    scenes = np.concatenate([synthetic_frame(s, 1080, 1920) for s in range(4)])
    data = np.tile(scenes.reshape(-1), (args.frames + 3) // 4)[:n]
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    k3, shift3 = vfilter.as_kernel(vfilter.kernels.gaussian3())
    centre = ((w - 1) / 2, (h - 1) / 2)
    maps = {"flip_h": Warp(flip="h", interpolation="nearest"),
            "shift_half": Warp(warps.translation(0.5, 0.5)),
            "rotate5_scale1.1": Warp(warps.rotation(centre, 5.0, 1.1)),
            "rotate30": Warp(warps.rotation(centre, 30.0, 1.0)),
            "shrink_0.5": Warp(warps.zoom(0.5, centre))}
    settings = [(b, ROWS) for b in args.lds] + [(LDS, r) for r in args.rows if r != ROWS]
    if args.cross:
        settings = [(b, r) for r in args.rows for b in args.lds]
    out = {"bytes": n, "frames": args.frames, "calls": args.calls, "rounds": args.rounds, "committed": {"lds": LDS, "rows": ROWS},
           "yardsticks": {}, "maps": {}}
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        d_src, d_out = ctx.alloc_device(n), ctx.alloc_device(n)
        ctx.upload(d_src, data, n)
        ctx.sync()

        def per_frame(fn, env=None):
            def call():
                for k, v in (env or {}).items():
                    os.environ[k] = str(v)
                for f in range(args.frames):
                    fn(d_src + f * one, d_out + f * one)
            return call

        variants = {("lut3",): per_frame(lambda s, d: ctx.lut_device(s, d, one, t3, c3)),
                    ("filter2d",): per_frame(lambda s, d: ctx.conv_device(s, d, w, h, 3, k3, shift3))}
        for name, f in maps.items():
            for lds, rows in settings:
                variants[(name, lds, rows)] = per_frame(lambda s, d, f=f: ctx.warp_device(s, d, w, h, 3, *f.args),
                                                        {"VF_WARP_LDS": lds, "VF_WARP_ROWS": rows})
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
        for d in (d_src, d_out):
            ctx.free_device(d)
    for k in ("VF_WARP_LDS", "VF_WARP_ROWS"):
        os.environ.pop(k, None)
    for key, xs in us.items():
        s = stats(xs)
        rec = {"us": s, "us_per_frame": s["median"] / args.frames}
        if len(key) == 1:
            out["yardsticks"][key[0]] = rec
        else:
            out["maps"].setdefault(key[0], {})[f"lds={key[1]},rows={key[2]}"] = rec
    lut3, conv = (out["yardsticks"][k]["us"]["median"] for k in ("lut3", "filter2d"))
    for name, recs in out["maps"].items():
        for rec in recs.values():
            rec["vs_lut3"] = rec["us"]["median"] / lut3
            rec["vs_filter2d"] = rec["us"]["median"] / conv
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
        with open(args.out + ".table", "w") as f:  # the same numbers as a table, us a frame
            cols = [f"lds={b},rows={r}" for b, r in settings]
            f.write("us a frame, median of %d rounds of %d calls over %d frames\n" % (args.rounds, args.calls, args.frames))
            f.write("%-18s" % "map" + "".join("%22s" % c for c in cols) + "\n")
            for name, recs in out["maps"].items():
                f.write("%-18s" % name + "".join("%22.2f" % recs[c]["us_per_frame"] for c in cols) + "\n")
            for k, rec in out["yardsticks"].items():
                f.write("%-18s%22.2f\n" % (k, rec["us_per_frame"]))


if __name__ == "__main__":
    main()
