#!/usr/bin/env python3
"""Kernel-only time of the convolution filter next to the table kernel, HBM-resident, same
buffers, same process (profiles/conv_raw_bench.txt, profiles/conv_jpeg_bench.txt).

    tools/conv_bench.py raw   [--frames 32] [--launches 200] [--rounds 7]
    tools/conv_bench.py jpeg  [--frames 32] [--iters 20] [--rounds 5] [--which conv,invert_unfused]
    tools/conv_bench.py probe [--frames 32]          # one launch per variant, to run under rocprofv3 --pmc
    tools/conv_bench.py pmc CSV [CSV ...]            # per-kernel sums of rocprofv3 counter_collection.csv files

raw    1080p x 32 frames in device memory, random content, filtered as ONE 1920 x (1080 * frames)
       x 3 image, so a launch covers the same bytes as the table kernel's one launch (per-frame
       launches differ by the border rows only; `frames32` times those for the 3 x 3).  Variants:
       3 x 3, 5 x 5 and 7 x 7 kernels with sum|K| <= 128, each in the wide (32-bit) and the narrow
       (packed 16-bit) arithmetic form (VF_CONV_FORM, read per call), and vf_lut_device -- the
       memory-bound yardstick at 2 bytes of traffic per output byte.  A measurement is `launches`
       back-to-back launches on the null stream between two device synchronises, host clock; a
       round takes every variant once, in turn; the figures are the median, min and max over the
       rounds after one warm-up round.
jpeg   vf_jpeg_bench_conv (gaussian3) against vf_jpeg_bench_invert with VF_JPEG_FUSE=0 -- the same
       pixel round trip without the filter -- on one batch of 1080p scene frames (q85, 4:2:2),
       alternating.  (The parent commit's figure beside it in profiles/conv_jpeg_bench.txt comes from
       that commit's own tree: VF_JPEG_FUSE=0 tools/lut_bench.py jpeg --which invert.)
No GPU, no number: every path here needs the device.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distributed-video-filter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _kernels():
    import numpy as np
    import vfilter
    from vfilter import kernels as K
    k5 = np.random.default_rng(3).integers(-5, 6, (5, 5))
    k7 = np.random.default_rng(4).integers(-2, 3, (7, 7))
    ks = {"3x3": vfilter.as_kernel(K.gaussian3()), "5x5": vfilter.as_kernel((k5, 2)), "7x7": vfilter.as_kernel((k7, 1))}
    for w, _ in ks.values():
        assert abs(w.astype(int)).sum() <= 128  # both forms hold them
    return ks


def _variants(ctx, frames, probe=False):
    import numpy as np
    import vfilter
    w, h = 1920, 1080 * frames
    n = w * h * 3
    d_src, d_out = ctx.alloc_device(n), ctx.alloc_device(n)
    ctx.upload(d_src, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), n)
    ctx.sync()
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    ks = _kernels()

    def conv(name, form, per_frame=False):
        wts, s = ks[name]

        def launch():
            os.environ["VF_CONV_FORM"] = form
            if per_frame:
                fb = 1920 * 1080 * 3
                for f in range(frames):
                    ctx.conv_device(d_src + f * fb, d_out + f * fb, 1920, 1080, 3, wts, s, 0)
            else:
                ctx.conv_device(d_src, d_out, w, h, 3, wts, s, 0)
        return launch

    variants = {"lut3": lambda: ctx.lut_device(d_src, d_out, n, t3, c3),
                "invert": lambda: ctx.invert_device(d_src, d_out, n)}
    for name in ks:
        for form in ("wide", "narrow"):
            variants[f"{name}/{form}"] = conv(name, form)
    if not probe:
        variants["3x3/narrow/frames32"] = conv("3x3", "narrow", per_frame=True)
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
        variants, n, bufs = _variants(ctx, args.frames, probe=True)
        for _ in range(2):
            for launch in variants.values():
                launch()
                ctx.sync()
        for d in bufs:
            ctx.free_device(d)
    return {"mode": "probe", "bytes": n, "variants": list(variants)}


def pmc(args):
    """Per kernel name, the LAST dispatch's counters from rocprofv3 counter_collection.csv files."""
    last = defaultdict(dict)
    ids = {}
    for path in args.csv:
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
            key = (path, name)
            did = int(r["Dispatch_Id"])
            if ids.get(key, -1) < did:
                ids[key] = did
                for c in [c for c in last[name] if c.startswith(path + ":")]:
                    del last[name][c]
            if did == ids[key]:
                k = path + ":" + r["Counter_Name"]
                last[name][k] = last[name].get(k, 0.0) + float(r["Counter_Value"])
    out = {}
    for name, d in last.items():
        c = defaultdict(float)
        for k, v in d.items():
            c[k.split(":")[-1]] += v
        row = dict(c)
        cyc = c.get("GRBM_GUI_ACTIVE", 0.0) / 8  # summed over the 8 XCDs
        if cyc:
            row["kernel_cycles"] = cyc
            row["valu_issue_frac"] = c.get("SQ_INSTS_VALU", 0.0) * 2 / (1024 * cyc)  # 2 cycles per wave64 op, 1024 SIMDs
            row["lds_active_frac"] = c.get("SQ_LDS_IDX_ACTIVE", 0.0) / (256 * cyc) if "SQ_LDS_IDX_ACTIVE" in c else None
        out[name] = row
    return {"mode": "pmc", "kernels": out}


def jpeg(args):
    import vfilter
    from oracle import jpeg as J
    from vfilter import kernels as K
    scenes = [J.synthetic_scene(s, 1080, 1920) for s in range(min(args.frames, 8))]
    jpgs = [J.encode(scenes[i % len(scenes)], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(args.frames)]
    which = args.which.split(",")
    res = {w: [] for w in which}
    g3, s3 = vfilter.as_kernel(K.gaussian3())
    g7, s7 = vfilter.as_kernel(K.gaussian7())
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=args.frames) as ctx:
        def run(w, iters):
            if w == "conv":
                return ctx.jpeg_bench_conv(jpgs, g3, s3, 0, 85, J.TJSAMP_422, 0, iters=iters)[0]
            if w == "conv7":
                return ctx.jpeg_bench_conv(jpgs, g7, s7, 0, 85, J.TJSAMP_422, 0, iters=iters)[0]
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
            "lib": os.environ.get("VFILTER_LIB", "in-tree"),
            "variants": {w: {"batch_ms": stats(r), "batch_ms_runs": r} for w, r in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "jpeg", "probe", "pmc"))
    ap.add_argument("csv", nargs="*")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--which", default="conv,invert_unfused",
                    help="jpeg: conv (gaussian3) | conv7 (gaussian7) | invert_unfused (VF_JPEG_FUSE=0) | invert")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 7 if args.mode == "raw" else 5
    out = {"raw": raw, "jpeg": jpeg, "probe": probe, "pmc": pmc}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
