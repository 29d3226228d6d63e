#!/usr/bin/env python3
"""Time of the colour-matrix kernel next to the 3-channel table kernel, same buffers, same process
(profiles/mix_raw_bench.txt).

    tools/mix_bench.py raw   [--frames 32] [--launches 100] [--rounds 7]
    tools/mix_bench.py probe [--frames 32]     # one launch per variant, for rocprofv3 --pmc

raw    1080p x 32 frames in device memory, random content, as one range of 1920 x 1080 x 32 pixels.
       Variants: lut3 (vf_lut_device with three tables: the yardstick, 2 bytes of traffic per output
       byte, as the matrix has), and vf_mix_device with the three forms of the kernel -- none (shift
       0: BGR <-> RGB with offsets), half_up (the gray preset) and half_even (sepia) -- each out of
       place and in place (dst == src), and the same six with VF_MIX_FORM=stride: the kernel form
       whose lanes each take their own 48-byte units, against the default coalesced form (DESIGN.md
       20.3).  A measurement is `launches` back-to-back launches on the
       null stream between two device synchronises, host clock; a round takes every variant once,
       in turn; median, min and max over the rounds after one warm-up round.
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


def _variants(ctx, frames):
    import numpy as np
    import vfilter
    from vfilter import Mix, colors
    n = 1920 * 1080 * frames * 3
    d_a, d_c, d_out = (ctx.alloc_device(n) for _ in range(3))
    ctx.upload(d_a, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), n)
    ctx.upload(d_c, np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8), n)
    ctx.sync()
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    swap = (np.array([[0, 0, 1, 10], [0, 1, 0, -10], [1, 0, 0, 0]]), 0)
    forms = {"none": Mix(swap), "half_up": colors.gray(), "half_even": Mix(colors.sepia())}
    variants = {"lut3": lambda: ctx.lut_device(d_a, d_out, n, t3, c3)}
    for form in ("mix", "stride"):
        for name, mix in forms.items():
            variants[form + "_" + name] = lambda m=mix: ctx.mix_device(d_a, d_out, n, *m.args)
            variants[form + "_" + name + "_in_place"] = lambda m=mix: ctx.mix_device(d_c, d_c, n, *m.args)
    return variants, n, (d_a, d_c, d_out)


def _select_form(name):
    """VF_MIX_FORM is read per launch: the stride_* variants run the other kernel form."""
    if name.startswith("stride_"):
        os.environ["VF_MIX_FORM"] = "stride"
    else:
        os.environ.pop("VF_MIX_FORM", None)


def raw(args):
    import vfilter
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=4) as ctx:
        variants, n, bufs = _variants(ctx, args.frames)
        us = {k: [] for k in variants}
        for rnd in range(args.rounds + 1):
            for name, launch in variants.items():
                _select_form(name)
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
    base = stats(us["lut3"])
    out["lut3_spread_us"] = base["max"] - base["min"]
    for name, xs in us.items():
        s = stats(xs)
        out["variants"][name] = {"us": s, "GBps_out": {k: n / v / 1e3 for k, v in s.items()},
                                 "time_vs_lut3": s["median"] / base["median"],
                                 "above_lut3_by_more_than_its_spread": s["median"] - base["median"] > out["lut3_spread_us"]}
    return out


def probe(args):
    """Each variant once (after one untimed warm-up launch each), for a counters-only profiler run."""
    import vfilter
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        variants, n, bufs = _variants(ctx, args.frames)
        for _ in range(2):
            for name, launch in variants.items():
                _select_form(name)
                launch()
                ctx.sync()
        for d in bufs:
            ctx.free_device(d)
    return {"mode": "probe", "bytes": n, "variants": list(variants)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "probe"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"raw": raw, "probe": probe}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
