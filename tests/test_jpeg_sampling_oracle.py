"""The oracle on the JPEG sampling layouts TurboJPEG cannot write, and libjpeg's colour-space rule.

tests/golden/jpeg_sampling/ (make_jpeg_sampling_golden.py) holds streams libjpeg-turbo wrote with
the per-component factors set directly -- every block count 4..10, luma that is not the densest
component, Cb and Cr sampled differently, expansion by 3 and 4 -- with libjpeg-turbo's own decode
of each as sha256.  The oracle must reproduce those without libjpeg (the GPU tests lean on it),
equal libjpeg-turbo on fresh frames where the library is there, refuse what libjpeg refuses
(over 10 blocks per MCU, factors that do not divide the maximum) and refuse, never mis-decode, a
three-component stream that libjpeg reads as RGB.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import _jpeg_sampling as S
from oracle import jpeg as J

UNSUPPORTED = "oracle status -4"  # VFO_JE_UNSUPPORTED


def _sha(a) -> str:
    return hashlib.sha256(a if isinstance(a, bytes) else a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def cases(golden_dir):
    d = os.path.join(golden_dir, "jpeg_sampling")
    out = json.load(open(os.path.join(d, "manifest.json")))["cases"]
    for c in out:
        c["jpeg"] = open(os.path.join(d, c["file"]), "rb").read()
    return out


def _need_libjpeg():
    ok, why = J.libjpeg_available()
    if not ok:
        pytest.skip("libjpeg-turbo (libjpeg.so.8) not loadable: " + why)


def test_manifest_covers_the_layouts(cases):
    """Both small frames for every factor set, block counts 4..10 all present, the medium
    frames, and the files are the ones the manifest hashed."""
    small = [c for c in cases if c["group"] == "small"]
    assert sorted(tuple(c["factors"]) for c in small) == sorted(S.FACTOR_SETS * 2)
    assert {c["blocks_per_mcu"] for c in small} == {4, 5, 6, 7, 8, 9, 10}
    # per component, the expansion (he, ve) the colour pass applies
    exp = [[(max(f[0::2]) // f[2 * k], max(f[1::2]) // f[2 * k + 1]) for k in range(3)] for f in S.FACTOR_SETS]
    assert {e[0] for x in exp for e in x} == {1, 2, 3, 4} and {e[1] for x in exp for e in x} == {1, 2, 3, 4}
    assert {(4, 2), (2, 4), (3, 2), (3, 1), (1, 3), (4, 1), (1, 4)} <= {e for x in exp for e in x}
    assert any(x[0] != (1, 1) for x in exp), "luma that is not the densest component"
    assert any(x[1] != x[2] for x in exp), "Cb and Cr sampled differently"
    assert any({(2, 1), (1, 2)} <= set(x) for x in exp), "h2v1-fancy and h1v2-fancy components in one frame"
    assert [tuple(c["factors"]) for c in cases if c["group"] == "medium"] == S.MEDIUM_SETS
    assert sum(1 for c in cases if c["group"] == "medium" and c["libjpeg_options"]) == 1
    for c in cases:
        assert _sha(c["jpeg"]) == c["jpeg_sha256"], c["file"]
        assert c["blocks_per_mcu"] == (S.blocks_per_mcu(c["factors"]) if len(c["factors"]) == 6 else 1)
    assert sum(len(c["jpeg"]) for c in cases) < 400 * 1024


def test_oracle_decode_hashes_to_libjpeg(cases):
    """Needs no libjpeg: the expected hashes are libjpeg-turbo's, recorded in the manifest."""
    n = 0
    for c in cases:
        if c["colorspace"] == "rgb":
            continue
        assert J.info(c["jpeg"])["h"] == c["factors"][0::2] and J.info(c["jpeg"])["v"] == c["factors"][1::2]
        assert _sha(J.decode(c["jpeg"], J.TJPF_BGR, 0)) == c["decoded_sha256"], c["file"]
        assert _sha(J.decode(c["jpeg"], J.TJPF_BGR, J.TJFLAG_FASTUPSAMPLE)) == c["decoded_fast_sha256"], c["file"]
        rgb = J.decode(c["jpeg"], J.TJPF_RGB, 0)
        assert np.array_equal(rgb[..., ::-1], J.decode(c["jpeg"], J.TJPF_BGR, 0)), c["file"]
        n += 1
    assert n == len(cases) - 3


@pytest.mark.parametrize("size", [(1, 1), (2, 5), (47, 3), (17, 13), (33, 100)])
def test_live_sweep_against_libjpeg(size):
    _need_libjpeg()
    h, w = size
    for i, f in enumerate(S.FACTOR_SETS):
        rng = np.random.default_rng(1000 * h + 10 * w + i)
        for kind, q in (("noise", 90), ("scene", 75)):
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if kind == "noise" else \
                J.synthetic_scene(int(rng.integers(1 << 30)), h, w)
            opt = {"restart_interval": 1 + i % 4, "optimize": True} if (i + h) % 3 == 0 else {}
            jpg = J.libjpeg_encode_factors(img, q, f, **opt)
            for fast in (False, True):
                got = J.decode(jpg, J.TJPF_BGR, J.TJFLAG_FASTUPSAMPLE if fast else 0)
                assert np.array_equal(got, J.libjpeg_decode(jpg, J.TJPF_BGR, fast)), (f, size, kind, fast)


def test_layouts_libjpeg_refuses_are_refused(cases):
    """Over 10 blocks per MCU (JERR_BAD_MCU_SIZE) and factors that do not divide the maximum
    (JERR_FRACTIONAL_SAMPLING): the oracle answers "unsupported" from the header alone."""
    base = next(c for c in cases if c["file"].startswith("small_222111_noise"))
    hdr = {"width": 71, "height": 40, "ncomp": 3}
    have = J.libjpeg_available()[0]
    assert all(S.blocks_per_mcu(f) > 10 for f in S.OVER_10_BLOCKS)
    assert all(S.blocks_per_mcu(f) <= 10 for f in S.FRACTIONAL)
    for f in S.OVER_10_BLOCKS + S.FRACTIONAL:
        bad = S.with_factors(base["jpeg"], f)
        with pytest.raises(ValueError, match=UNSUPPORTED):
            J.info(bad)
        with pytest.raises(ValueError, match=UNSUPPORTED):
            J.decode(bad)
        if have:
            with pytest.raises(RuntimeError):
                J.libjpeg_decode(bad, J.TJPF_BGR, False, hdr)
    if have:
        for f in S.OVER_10_BLOCKS:
            with pytest.raises(ValueError, match="refuses"):
                J.libjpeg_encode_factors(np.zeros((16, 16, 3), np.uint8), 85, f)
    # the patch itself is sound: the stream's own factors written back decode as before
    same = S.with_factors(base["jpeg"], base["factors"])
    assert same == base["jpeg"]


def _app(marker: int, body: bytes) -> bytes:
    n = len(body) + 2
    return bytes([0xFF, marker, n >> 8, n & 255]) + body


def _adobe(transform: int, n: int = 12) -> bytes:
    return _app(0xEE, (b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))[:n] + b"\x00" * max(0, n - 12))


JFIF = _app(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def _space_variants(cases):
    """(name, stream, colour space by the rule) -- the fixtures, and streams crafted from the
    marker-less YCbCr one by inserting APPn segments after SOI and renaming the components."""
    by = {c["file"]: c for c in cases}
    out = [(c["file"], c["jpeg"], c["colorspace"]) for c in cases if c["group"] == "space"]
    plain = by["space_ycc_no_marker_ids_012.jpg"]["jpeg"]
    ins = lambda *segs: plain[:2] + b"".join(segs) + plain[2:]  # noqa: E731
    out += [
        ("adobe0", ins(_adobe(0)), "rgb"),
        ("adobe1", ins(_adobe(1)), "ycc"),
        ("adobe2", ins(_adobe(2)), "ycc"),       # YCCK's value on three components: libjpeg warns, YCbCr
        ("adobe255", ins(_adobe(255)), "ycc"),
        ("adobe0_long", ins(_adobe(0, 40)), "rgb"),
        ("adobe0_short", ins(_adobe(0, 11)), "ycc"),  # under 12 data bytes: not an Adobe marker
        ("adobe0_short_ids_rgb", S.with_ids(ins(_adobe(0, 11)), b"RGB"), "rgb"),
        ("adobe_twice_last_wins_1", ins(_adobe(0), _adobe(1)), "ycc"),
        ("adobe_twice_last_wins_0", ins(_adobe(1), _adobe(0)), "rgb"),
        ("adobe0_then_jfif", ins(_adobe(0), JFIF), "ycc"),  # JFIF outranks Adobe wherever it stands
        ("jfif_then_adobe0", ins(JFIF, _adobe(0)), "ycc"),
        ("jfif_short_adobe0", ins(_app(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00"), _adobe(0)), "rgb"),
        ("jfxx_adobe0", ins(_app(0xE0, b"JFXX\x00\x10" + b"\x00" * 10), _adobe(0)), "rgb"),
        ("app14_not_adobe", ins(_app(0xEE, b"adobe\x00\x64\x00\x00\x00\x00\x00")), "ycc"),
        ("adobe_in_app13", ins(_app(0xED, b"Adobe\x00\x64\x00\x00\x00\x00\x00")), "ycc"),
        ("ids_RGB", S.with_ids(plain, b"RGB"), "rgb"),
        ("ids_RGb", S.with_ids(plain, b"RGb"), "ycc"),
        ("ids_BGR", S.with_ids(plain, b"BGR"), "ycc"),
        ("ids_123", S.with_ids(plain, (1, 2, 3)), "ycc"),
        ("ids_RGB_jfif", S.with_ids(ins(JFIF), b"RGB"), "ycc"),
        ("ids_RGB_adobe1", S.with_ids(ins(_adobe(1)), b"RGB"), "ycc"),
    ]
    # the Adobe marker between SOF and SOS counts too (read_markers runs to SOS)
    sos = plain.index(b"\xff\xda")
    out.append(("adobe0_before_sos", plain[:sos] + _adobe(0) + plain[sos:], "rgb"))
    return out


def test_colour_space_rule(cases):
    """jdapimin.c default_decompress_parms on three components: a JFIF APP0 seen -> YCbCr; else
    an Adobe APP14 (12 data bytes, "Adobe") -> transform 0 is RGB, anything else YCbCr; else ids
    'R','G','B' -> RGB, anything else YCbCr.  One component is gray.  Pinned against libjpeg-turbo
    where it is there; the oracle refuses exactly the RGB streams (decoded as YCbCr they differ
    from libjpeg by up to 248 per channel) and decodes the others to libjpeg's pixels; the
    product's host parse (vf_jpeg_header, no GPU) names the same colour space."""
    from vfilter._lib import jpeg_header
    from vfilter.jpeg import TJCS_GRAY, TJCS_RGB, TJCS_YCbCr
    have = J.libjpeg_available()[0]
    tjcs = {"rgb": TJCS_RGB, "ycc": TJCS_YCbCr, "gray": TJCS_GRAY}
    variants = _space_variants(cases)
    assert sum(1 for v in variants if v[2] == "rgb") >= 10
    for name, jpg, want in variants:
        if have:
            assert J.libjpeg_colorspace(jpg) == want, name
        assert jpeg_header(jpg)[3] == tjcs[want], name
        if want == "rgb":
            with pytest.raises(ValueError, match=UNSUPPORTED):
                J.info(jpg)
            with pytest.raises(ValueError, match=UNSUPPORTED):
                J.decode(jpg)
        elif have:
            for fast in (False, True):
                assert np.array_equal(J.decode(jpg, J.TJPF_BGR, J.TJFLAG_FASTUPSAMPLE if fast else 0),
                                      J.libjpeg_decode(jpg, J.TJPF_BGR, fast)), name


def test_patched_gray_frames_decode_alike(cases):
    """One component: a non-interleaved scan has one block per MCU whatever the SOF's sampling
    byte says, so 0x22, 0x41, 0x33 and 0x14 decode like the 0x11 original."""
    gray = [c for c in cases if c["file"].startswith("space_gray")]
    assert len(gray) == 5 and len({c["decoded_sha256"] for c in gray}) == 1
    for c in gray:
        assert _sha(J.decode(c["jpeg"])) == c["decoded_sha256"]


def test_remuxed_headers_decode_like_the_original(golden_dir):
    """A 4:2:2 DRI stream with its header rewritten (DHTs merged, DQTs split and moved past SOF;
    DQTs merged, DHTs reordered; DRI before SOF; a 65,533-byte APP1 full of marker look-alikes
    and a COM; 0xFF fill bytes before markers): entropy bytes kept, so libjpeg-turbo's decode of
    the original (tests/golden/jpeg/manifest.json) is the expected one."""
    d = os.path.join(golden_dir, "jpeg")
    case = {c["file"]: c for c in json.load(open(os.path.join(d, "manifest.json")))["cases"]}[S.REMUX_BASE]
    jpg = open(os.path.join(d, S.REMUX_BASE), "rb").read()
    muxes = S.remuxes(jpg)
    assert len({m for _, m in muxes} | {jpg}) == len(muxes) + 1
    have = J.libjpeg_available()[0]
    for name, m in muxes:
        assert m[m.rindex(b"\xff\xda"):][14:] == jpg[jpg.rindex(b"\xff\xda"):][14:], name
        assert _sha(J.decode(m)) == case["decoded_sha256"], name
        assert J.info(m)["restart_interval"] == 2, name
        if have:
            assert _sha(J.libjpeg_decode(m)) == case["decoded_sha256"], name
