#!/usr/bin/env python3
"""Time of the binary kernel and of filter chains next to their parts, same buffers, same process
(profiles/chain_raw_bench.txt, profiles/chain_jpeg_bench.txt).

    tools/chain_bench.py raw   [--frames 32] [--launches 100] [--rounds 7]
    tools/chain_bench.py jpeg  [--frames 32] [--iters 20] [--rounds 5]
    tools/chain_bench.py probe [--frames 32]     # one launch per device variant, for rocprofv3 --pmc

raw    1080p x 32 frames in device memory, random content, as ONE 1920 x (1080 * frames) x 3 image.
       Device variants: lut3 (vf_lut_device, 2 bytes of traffic per output byte), the five binary
       ops (vf_binary_device, 3 bytes per output byte), the same in place (dst == a), erode3 and
       dilate3 (vf_rank_device, rect3), and gradient_seq: dilate3, erode3 and subtract queued back
       to back, the launches the `gradient` rect3 program makes, against the sum of the three
       measured alone.  A measurement is `launches` back-to-back launches (gradient_seq: sequences)
       on the null stream between two device synchronises, host clock; a round takes every variant
       once, in turn; median, min and max over the rounds after one warm-up round.
       Host variants (`--host-calls` calls per measurement): the same frames through
       vf_rank_frames_host (erode rect3) and vf_chain_frames_host (gradient rect3), which share
       the upload, the download and the band loop; the difference is what the program's two further
       kernels and its scratch cost on that path.
jpeg   vf_jpeg_bench_chain for open3, gradient rect3 and edges against vf_jpeg_bench_rank erode rect3
       and the unfused inversion (VF_JPEG_FUSE=0: the pixel round trip without a filter) on one
       batch of 1080p scene frames (q85, 4:2:2), alternating.
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

OPS = ("subtract", "add", "absdiff", "min", "max")


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _device_variants(ctx, frames):
    import numpy as np
    import vfilter
    from vfilter import Rank, elements
    from vfilter.filters import BINARY_OPS
    w, h = 1920, 1080 * frames
    n = w * h * 3
    d_a, d_b, d_c, d_out = (ctx.alloc_device(n) for _ in range(4))
    ctx.upload(d_a, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), n)
    ctx.upload(d_b, np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8), n)
    ctx.sync()
    perm = lambda s: np.random.default_rng(s).permutation(256).astype(np.uint8)  # noqa: E731
    t3, c3 = vfilter.as_table(vfilter.tables.stack(perm(2), perm(3), perm(4)))
    ero, dil = Rank.erode(elements.rect(3)), Rank.dilate(elements.rect(3))
    variants = {"lut3": lambda: ctx.lut_device(d_a, d_out, n, t3, c3)}
    for op in OPS:
        variants[op] = lambda code=BINARY_OPS[op]: ctx.binary_device(d_a, d_b, d_out, n, code)
    variants["subtract_in_place"] = lambda: ctx.binary_device(d_c, d_b, d_c, n, BINARY_OPS["subtract"])
    variants["erode3"] = lambda: ctx.rank_device(d_a, d_out, w, h, 3, *ero.args)
    variants["dilate3"] = lambda: ctx.rank_device(d_a, d_c, w, h, 3, *dil.args)

    def gradient_seq():
        ctx.rank_device(d_a, d_c, w, h, 3, *dil.args)
        ctx.rank_device(d_a, d_out, w, h, 3, *ero.args)
        ctx.binary_device(d_c, d_out, d_c, n, BINARY_OPS["subtract"])

    variants["gradient_seq"] = gradient_seq
    return variants, n, (d_a, d_b, d_c, d_out)


def raw(args):
    import numpy as np
    import vfilter
    from vfilter import Rank, elements
    from vfilter.filters import Morph
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=4) as ctx:
        variants, n, bufs = _device_variants(ctx, args.frames)
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
        # the host path: the same frames, separately stored, through the *_frames_host calls
        rng = np.random.default_rng(5)
        frames = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(args.frames)]
        outs = [np.empty_like(f) for f in frames]
        ws, hs = [1920] * args.frames, [1080] * args.frames
        ero, grad = Rank.erode(elements.rect(3)), Morph("gradient", elements.rect(3))
        host = {"host_erode3": lambda: ctx.rank_frames_host(frames, outs, ws, hs, 3, *ero.args),
                "host_gradient3": lambda: ctx.chain_frames_host(frames, outs, ws, hs, 3, *grad.args)}
        hms = {k: [] for k in host}
        for rnd in range(args.rounds + 1):
            for name, call in host.items():
                t0 = time.perf_counter()
                for _ in range(args.host_calls):
                    call()
                if rnd:
                    hms[name].append((time.perf_counter() - t0) / args.host_calls * 1e3)
    out = {"mode": "raw", "bytes": n, "launches": args.launches, "rounds": args.rounds, "variants": {}, "host": {}}
    base = statistics.median(us["lut3"])
    for name, xs in us.items():
        s = stats(xs)
        out["variants"][name] = {"us": s, "GBps_out": {k: n / v / 1e3 for k, v in s.items()},
                                 "time_vs_lut3": s["median"] / base}
    parts = [statistics.median(us[k]) for k in ("dilate3", "erode3", "subtract_in_place")]
    out["gradient"] = {"seq_us": stats(us["gradient_seq"]), "sum_of_parts_us": sum(parts),
                       "seq_vs_sum": statistics.median(us["gradient_seq"]) / sum(parts)}
    for name, xs in hms.items():
        out["host"][name] = {"call_ms": stats(xs), "frame_us": statistics.median(xs) / args.frames * 1e3}
    return out


def probe(args):
    """Each device variant once (after one untimed warm-up launch each), for a counters-only profiler run."""
    import vfilter
    with vfilter.Context(0, max_frame_bytes=1 << 20) as ctx:
        variants, n, bufs = _device_variants(ctx, args.frames)
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
    from vfilter import Rank, elements, tables
    from vfilter.filters import Chain, Morph, Table
    scenes = [J.synthetic_scene(s, 1080, 1920) for s in range(min(args.frames, 8))]
    jpgs = [J.encode(scenes[i % len(scenes)], 85, J.TJPF_BGR, J.TJSAMP_422) for i in range(args.frames)]
    r3 = elements.rect(3)
    chains = {"open3": Morph("open", r3), "gradient3": Morph("gradient", r3),
              "edges": Chain([Rank.median(3), Morph("gradient", r3), Table(tables.threshold(24))])}
    which = ["erode3", "open3", "gradient3", "edges", "invert_unfused"]
    res = {w: [] for w in which}
    with vfilter.Context(0, max_frame_bytes=1920 * 1080 * 3, max_batch=args.frames) as ctx:
        def run(w, iters):
            if w == "invert_unfused":  # the pixel round trip (VF_JPEG_FUSE is read per call)
                os.environ["VF_JPEG_FUSE"] = "0"
                try:
                    return ctx.jpeg_bench_invert(jpgs, 85, J.TJSAMP_422, 0, iters=iters)[0]
                finally:
                    del os.environ["VF_JPEG_FUSE"]
            if w == "erode3":
                return ctx.jpeg_bench_rank(jpgs, *Rank.erode(r3).args, 85, J.TJSAMP_422, 0, iters=iters)[0]
            return ctx.jpeg_bench_chain(jpgs, *chains[w].args, 85, J.TJSAMP_422, 0, iters=iters)[0]
        for rnd in range(args.rounds + 1):
            for w in which:
                ms = run(w, 2 if rnd == 0 else args.iters)
                if rnd:
                    res[w].append(ms)
    base = statistics.median(res["invert_unfused"])
    return {"mode": "jpeg", "frames": args.frames, "iters": args.iters, "rounds": args.rounds,
            "variants": {w: {"batch_ms": stats(r), "steps": len(chains[w]) if w in chains else (1 if w == "erode3" else 0),
                             "filter_us_per_frame": (statistics.median(r) - base) / args.frames * 1e3}
                         for w, r in res.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("raw", "jpeg", "probe"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
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
