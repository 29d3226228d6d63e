#!/usr/bin/env python3
"""Make the JPEG fixtures in tests/golden/jpeg_sampling/ (run in the build container).

TurboJPEG can write five sampling layouts (TJSAMP_444 / 422 / 420 / GRAY / 440); a baseline
decoder meets any three-component frame whose factors are 1..4, divide their maxima and give
at most 10 blocks per MCU.  These fixtures cover that space, and the colour-space markers a
decoder has to read before it may treat three components as YCbCr.  As in make_jpeg_golden.py,
every stream is written and every expected decode is computed by the image's libjpeg-turbo
2.1.2 (libjpeg.so.8) through oracle/jpeg_xcheck.c -- here its xc_encode_factors, which sets the
per-component factors TJSAMP_* cannot name -- not by the oracle or the product:

  small/   every set of tests/_jpeg_sampling.py FACTOR_SETS: a 17 x 13 scene and a 40 x 71
           noise frame (neither a whole number of MCUs in either direction)
  medium/  six sets, ~120 x 168 noise at q95, 20-40 KB: several workgroups of the Huffman
           synchronisation per frame; one with DRI 3 and optimised tables
  space/   ~35 x 50: RGB-space streams (Adobe transform 0; ids 'R','G','B' with no marker),
           YCbCr streams that only the rule identifies (Adobe transform 1; JFIF with ids
           R, G, B; no marker with ids 0,1,2 and 'Y','C','c'), and a gray frame whose SOF
           sampling byte says 0x22, 0x41, 0x33, 0x14

manifest.json per case: file, factors, blocks per MCU, libjpeg's colour space, sha256 of the
JPEG, sha256 of libjpeg-turbo's BGR decode with fancy and with replicating upsampling.

    python tests/golden/make_jpeg_sampling_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import _jpeg_sampling as S  # noqa: E402
from oracle import jpeg as J  # noqa: E402

OUT = os.path.join(HERE, "jpeg_sampling")


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def sha(b) -> str:
    return hashlib.sha256(b if isinstance(b, bytes) else b.tobytes()).hexdigest()


def main():
    ok, why = J.libjpeg_available()
    if not ok:
        sys.exit(f"libjpeg-turbo not usable: {why}")
    os.makedirs(OUT, exist_ok=True)
    cases = []

    def add(group, name, jpg, factors, shape, ncomp=3, **extra):
        fn = f"{group}_{name}.jpg"
        with open(os.path.join(OUT, fn), "wb") as f:
            f.write(jpg)
        hdr = {"width": shape[1], "height": shape[0], "ncomp": ncomp}
        cases.append({
            "file": fn, "group": group, "factors": list(factors), "blocks_per_mcu": S.blocks_per_mcu(factors)
            if ncomp == 3 else 1, "shape": [shape[0], shape[1], 3], "colorspace": J.libjpeg_colorspace(jpg),
            "bytes": len(jpg), "jpeg_sha256": sha(jpg),
            "decoded_sha256": sha(J.libjpeg_decode(jpg, J.TJPF_BGR, False, hdr)),
            "decoded_fast_sha256": sha(J.libjpeg_decode(jpg, J.TJPF_BGR, True, hdr)), **extra})

    for i, f in enumerate(S.FACTOR_SETS):
        add("small", f"{S.name_of(f)}_scene_17x13", J.libjpeg_encode_factors(J.synthetic_scene(100 + i, 17, 13), 85, f),
            f, (17, 13))
        add("small", f"{S.name_of(f)}_noise_40x71", J.libjpeg_encode_factors(noise(200 + i, 40, 71), 60, f), f, (40, 71))
    for i, f in enumerate(S.MEDIUM_SETS):
        # (2,2, 2,1, 2,1): 8 blocks per MCU, so it rides the LSB-first lanes; over 32 KiB of
        # entropy-coded data, more than a span-sync workgroup covers at 4 subsequences per thread
        h, w = (136, 184) if i == 1 else (120, 168)
        opt = {"restart_interval": 3, "optimize": True} if i == 2 else {}
        add("medium", f"{S.name_of(f)}_noise_{h}x{w}", J.libjpeg_encode_factors(noise(300 + i, h, w), 95, f, **opt), f,
            (h, w), libjpeg_options=opt)

    img = J.synthetic_scene(400, 35, 50)
    f422 = (2, 1, 1, 1, 1, 1)
    enc = J.libjpeg_encode_factors
    plain = enc(img, 85, f422, jfif=False)
    f444 = (1, 1, 1, 1, 1, 1)
    for name, f, jpg in [
        ("rgb_adobe0", f444, enc(img, 85, f444, colorspace="rgb", jfif=False, adobe=True)),
        ("rgb_ids_no_marker", f444, enc(img, 85, f444, colorspace="rgb", jfif=False, adobe=False)),
        ("rgb_adobe0_422", f422, enc(img, 85, f422, colorspace="rgb", jfif=False, adobe=True)),
        ("ycc_adobe1_no_jfif", f422, enc(img, 85, f422, jfif=False, adobe=True)),
        ("ycc_jfif_ids_rgb", f422, S.with_ids(enc(img, 85, f422), b"RGB")),
        # JFIF outranks the Adobe marker: RGB samples that libjpeg reads as YCbCr all the same
        ("ycc_jfif_and_adobe0", f422, enc(img, 85, f422, colorspace="rgb", jfif=True, adobe=True)),
        ("ycc_no_marker_ids_012", f422, S.with_ids(plain, (0, 1, 2))),
        ("ycc_no_marker_ids_Ycc", f422, S.with_ids(plain, b"YCc")),
        ("ycc_no_marker_ids_rgb_lower", f422, S.with_ids(plain, b"rgb")),
    ]:
        add("space", name, jpg, f, (35, 50))
    gray = J.libjpeg_encode(img, 85, J.TJPF_BGR, J.TJSAMP_GRAY)
    for hv in (0x11, 0x22, 0x41, 0x33, 0x14):
        add("space", f"gray_sof_{hv:02x}", S.with_gray_sampling(gray, hv), (hv >> 4, hv & 15), (35, 50), ncomp=1)

    want = {"rgb": ("rgb_",), "ycc": ("ycc_", "small", "medium"), "gray": ("gray_",)}
    for c in cases:  # libjpeg's verdict is the one each file's name states
        key = c["file"].split("_", 1)[1] if c["group"] == "space" else c["group"]
        assert key.startswith(want[c["colorspace"]]), (c["file"], c["colorspace"])
    gh = {c["decoded_sha256"] for c in cases if c["file"].startswith("space_gray")}
    assert len(gh) == 1, "libjpeg decodes the patched gray frames like the original"
    total = sum(c["bytes"] for c in cases)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump({"generator": "libjpeg-turbo 2.1.2 (libjpeg.so.8) via oracle/jpeg_xcheck.c xc_encode_factors; "
                                "tests/golden/make_jpeg_sampling_golden.py", "libjpeg": why, "cases": cases}, f, indent=1)
    print(f"wrote {len(cases)} cases, {total} bytes of JPEG, to {OUT}")


if __name__ == "__main__":
    main()
