"""The gfx950 JPEG decoder on sampling layouts TurboJPEG cannot write, and on colour spaces.

The host parse (csrc/vf_jpeg_parse.h parse / make_geom) takes any three-component frame whose
factors are 1..4, divide their maxima and give at most 10 blocks per MCU -- libjpeg's own rule --
while tests/test_gpu_jpeg.py decodes only the five TJSAMP_* layouts.  The fixtures of
tests/golden/jpeg_sampling/ (libjpeg-turbo-made, make_jpeg_sampling_golden.py) reach the rest:

  * the colour pass's general upsampling (expansion by 3 and 4, luma that is not the densest
    component, Cb and Cr sampled differently, h2v1-fancy and h1v2-fancy components in one frame),
    the per-frame layout word and the batch-common one;
  * block cycles of 5, 7, 8, 9 and 10 in the write pass, the span sync and the speculative sync,
    and cycles of 4 (Y, Cb, Cb, Cr) and 8 on the LSB-first lanes, which had only seen
    Y, Y, Cb, Cr and gray.

Everything is exact: pixels against the oracle (pinned to libjpeg-turbo on these layouts by
tests/test_jpeg_sampling_oracle.py) and against libjpeg-turbo's own hashes in the manifest,
re-encoded bytes against the oracle's.  No test here needs libjpeg or anything outside tests/.
Streams libjpeg would read as RGB, or refuse for their layout, must raise from the host parse
(Codec::prepare_decode returns on a parse error before anything is staged or launched).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import _jpeg_sampling as S
from oracle import jpeg as J
from vfilter import VFilterError
from vfilter.jpeg import TJCS_GRAY, TJCS_RGB, TJCS_YCbCr, TJFLAG_FASTUPSAMPLE, TurboJPEG

pytestmark = pytest.mark.gpu

SWITCHES = ("VF_JPEG_SYNC", "VF_JPEG_SYNC_LSB", "VF_JPEG_SYNC_TABS4", "VF_JPEG_SYNC_G", "VF_JPEG_SYNC_QUEUED",
            "VF_JPEG_SYNC_WARM", "VF_JPEG_CHUNKS", "VF_JPEG_WRITE4", "VF_JPEG_FUSE", "VF_JPEG_FUSE_IDCT", "VF_JPEG_IDCT24")


def _sha(a) -> str:
    return hashlib.sha256(a if isinstance(a, bytes) else a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def tj(vf_ctx):
    return TurboJPEG(ctx=vf_ctx)


@pytest.fixture(scope="module")
def cases(golden_dir):
    d = os.path.join(golden_dir, "jpeg_sampling")
    out = json.load(open(os.path.join(d, "manifest.json")))["cases"]
    for c in out:
        c["jpeg"] = open(os.path.join(d, c["file"]), "rb").read()
        assert _sha(c["jpeg"]) == c["jpeg_sha256"], c["file"]
    return out


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


# the oracle's answers, computed once per (stream, settings) and shared by every test
_dec, _inv = {}, {}


def want_pixels(j, pf=J.TJPF_BGR, flags=0):
    k = (j, pf, flags)
    if k not in _dec:
        _dec[k] = J.decode(j, pf, flags)
        _dec[k].setflags(write=False)
    return _dec[k]


def want_invert(j, out_ss=J.TJSAMP_422, flags=0):
    k = (j, out_ss, flags)
    if k not in _inv:
        _inv[k] = J.encode(np.bitwise_not(want_pixels(j, J.TJPF_BGR, flags)), 85, J.TJPF_BGR, out_ss, flags)
    return _inv[k]


def _check_invert(tj, batch, note, out_ss=J.TJSAMP_422, flags=0):
    got = tj.invert_batch(batch, 85, out_ss, flags)
    assert len(got) == len(batch)
    for i, (g, j) in enumerate(zip(got, batch)):
        assert bytes(g) == want_invert(j, out_ss, flags), (note, i, J.info(j), out_ss, flags)


def _group(cases, group):
    return [c for c in cases if c["group"] == group]


def _standard(kind, i, h, w, ss, q=85):
    img = np.random.default_rng(700 + i).integers(0, 256, (h, w, 3), dtype=np.uint8) if kind == "noise" else \
        J.synthetic_scene(700 + i, h, w)
    return J.encode(img, q, J.TJPF_BGR, ss)


def _entropy_bytes(j) -> int:
    return len(j) - list(S.segments(j))[-1][2] - 2  # SOS end .. EOI


@pytest.mark.parametrize("flags", [0, TJFLAG_FASTUPSAMPLE])
def test_decode_every_fixture(tj, cases, flags):
    """tj.decode, fancy and replicating, BGR and RGB, of every fixture libjpeg reads as YCbCr or
    gray -- alone and all in one decode_batch -- against the oracle's pixels, and the BGR ones
    against libjpeg-turbo's own hash."""
    good = [c for c in cases if c["colorspace"] != "rgb"]
    assert len(good) == 2 * len(S.FACTOR_SETS) + len(S.MEDIUM_SETS) + 6 + 5
    key = "decoded_fast_sha256" if flags else "decoded_sha256"
    for c in good:
        for pf in (J.TJPF_BGR, J.TJPF_RGB):
            got = tj.decode(c["jpeg"], pf, flags=flags)
            assert got.shape == tuple(c["shape"])
            assert np.array_equal(got, want_pixels(c["jpeg"], pf, flags)), (c["file"], pf, flags)
            if pf == J.TJPF_BGR:
                assert _sha(got) == c[key], c["file"]
    for got, c in zip(tj.decode_batch([c["jpeg"] for c in good], J.TJPF_BGR, flags), good):
        assert _sha(got) == c[key], c["file"]


def test_header_reports_the_turbojpeg_sampling(tj, cases):
    """vf_jpeg_header's subsampling: TJSAMP_411 (5) for 4 x 1 luma over 1 x 1 chroma, -1 for every
    other layout TurboJPEG has no name for; its colour space is libjpeg's verdict."""
    seen = []
    for c in cases:
        w, h, ss, cs = tj.decode_header(c["jpeg"])
        assert (h, w) == tuple(c["shape"][:2])
        assert cs == {"ycc": TJCS_YCbCr, "rgb": TJCS_RGB, "gray": TJCS_GRAY}[c["colorspace"]], c["file"]
        if c["group"] == "small":
            assert ss == S.tjsamp_of(c["factors"]), c["file"]
            seen.append(ss)
        elif c["colorspace"] == "gray":
            assert ss == J.TJSAMP_GRAY
    assert seen.count(5) == 2 and seen.count(-1) == len(seen) - 2


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("factors", S.FACTOR_SETS, ids=S.name_of)
def test_invert_uniform_batch(tj, cases, monkeypatch, factors, fuse):
    """Each layout alone: the batch-common layout word is the frame's (0 for all of these, the
    general kernel), every frame has the same block cycle.  Into 4:2:2 (one-row colour pass) and
    4:2:0 (two rows), fancy and replicating, fused into the encoder's planes and through pixels."""
    monkeypatch.setenv("VF_JPEG_FUSE", fuse)
    batch = [c["jpeg"] for c in cases if c["group"] in ("small", "medium") and tuple(c["factors"]) == factors]
    assert len(batch) in (2, 3)
    batch = batch + batch[:1]
    for out_ss in (J.TJSAMP_422, J.TJSAMP_420):
        for flags in (0, TJFLAG_FASTUPSAMPLE):
            _check_invert(tj, batch, S.name_of(factors), out_ss, flags)


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("out_ss", [J.TJSAMP_422, J.TJSAMP_420])
def test_invert_mixed_batches(tj, cases, monkeypatch, out_ss, fuse):
    """All small fixtures in one batch (23 layouts, cycles 4..10: no common layout word, no
    LSB-first lane), and the general layouts interleaved with standard 4:2:2 and 4:2:0 frames
    (the batch is neither all-4:2:2 nor uniform, and the standard frames' specialised colour
    branches run next to the general one)."""
    monkeypatch.setenv("VF_JPEG_FUSE", fuse)
    small = [c["jpeg"] for c in _group(cases, "small")]
    for flags in (0, TJFLAG_FASTUPSAMPLE):
        _check_invert(tj, small, "all small", out_ss, flags)
    std = [_standard("scene", 0, 17, 13, J.TJSAMP_422), _standard("noise", 1, 64, 48, J.TJSAMP_420),
           _standard("scene", 2, 31, 45, J.TJSAMP_420), _standard("noise", 3, 40, 71, J.TJSAMP_422)]
    mixed = []
    for i, j in enumerate(small[::3]):
        mixed += [j, std[i % 4]]
    _check_invert(tj, mixed, "interleaved", out_ss, 0)
    _check_invert(tj, mixed[::-1], "interleaved reversed", out_ss, TJFLAG_FASTUPSAMPLE)


def _pow2_batch(cases):
    """Only block cycles that divide 16: the general 4- and 8-block layouts (Y, Cb, Cb, Cr;
    Y x 4, Cb x 2, Cr x 2; Y x 6, Cb, Cr), standard 4:2:2 and gray."""
    gen = [c["jpeg"] for c in cases if c["group"] in ("small", "medium") and c["blocks_per_mcu"] in (4, 8)]
    assert len(gen) == 2 * 6 + 3
    return gen + [_standard("noise", 4, 72, 100, J.TJSAMP_422, 92), _standard("scene", 5, 90, 121, J.TJSAMP_GRAY),
                  _standard("scene", 6, 17, 13, J.TJSAMP_422)]


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("lsb", ["1", "0"])
@pytest.mark.parametrize("sync", ["spec", "pass"])
def test_invert_power_of_two_cycles(tj, cases, monkeypatch, sync, lsb, fuse):
    """A batch whose every block cycle divides 16 takes the syncs' LSB-first lanes, whose slot
    patterns are built from the cycle: here Y,Cb,Cb,Cr and the 8-block general layouts next to
    Y,Y,Cb,Cr and gray.  Equal to the MSB-first lanes (VF_JPEG_SYNC_LSB=0) and to the oracle."""
    monkeypatch.setenv("VF_JPEG_SYNC", sync)
    monkeypatch.setenv("VF_JPEG_SYNC_LSB", lsb)
    monkeypatch.setenv("VF_JPEG_FUSE", fuse)
    batch = _pow2_batch(cases)
    for out_ss in (J.TJSAMP_422, J.TJSAMP_420):
        _check_invert(tj, batch, "pow2", out_ss, 0)
    _check_invert(tj, [j for j in batch if J.info(j)["ncomp"] == 3 and J.info(j)["h"][0] == 1], "Y,Cb,Cb,Cr only")


def _sync_params():
    out = []
    for sync in ("spec", "pass"):
        for g in ("1", None, "4"):
            if g == "4" and sync == "spec":
                continue  # the span width is the pass-based sync's
            for lsb in ("1", "0"):
                for tabs4 in ("1", "0"):
                    for chunks in ("1", "0"):
                        out.append(pytest.param(sync, g, lsb, tabs4, chunks,
                                                id=f"{sync}-g{g or 'dflt'}-lsb{lsb}-tabs{tabs4}-chunks{chunks}"))
    return out


@pytest.mark.parametrize("sync,g,lsb,tabs4,chunks", _sync_params())
def test_medium_frames_across_sync_workgroups(tj, cases, monkeypatch, sync, g, lsb, tabs4, chunks):
    """The medium frames (20-40 KB of noise at q95) span several workgroups of either sync: a
    span-sync workgroup covers 256 threads x G subsequences x 32 bytes (8 KiB at G = 1, 32 KiB at
    G = 4, which only the 8-block (2,2, 2,1, 2,1) frame exceeds -- G = 4 and 5 are the widths with
    the four-table LSB-first lane), a speculative one 256 / lanes(cycle) subsequences (at most
    8 KiB).  Two batches: all six (cycles 4, 8, 8, 6, 7, 10: MSB-first lanes) and the 4- and
    8-block ones with standard 4:2:2 and gray (LSB-first lanes when VF_JPEG_SYNC_LSB allows).
    One frame carries DRI 3 and optimised tables (its segments are 3 MCUs each)."""
    monkeypatch.setenv("VF_JPEG_SYNC", sync)
    monkeypatch.setenv("VF_JPEG_SYNC_LSB", lsb)
    monkeypatch.setenv("VF_JPEG_SYNC_TABS4", tabs4)
    monkeypatch.setenv("VF_JPEG_CHUNKS", chunks)
    if g:
        monkeypatch.setenv("VF_JPEG_SYNC_G", g)
    med = _group(cases, "medium")
    whole = [c for c in med if not c["libjpeg_options"]]
    assert len(med) == 6 and len(whole) == 5
    if sync == "spec" or g == "1":
        assert all(_entropy_bytes(c["jpeg"]) > 2 * 8192 for c in whole), [len(c["jpeg"]) for c in whole]
    if g == "4":
        assert any(_entropy_bytes(c["jpeg"]) > 32768 and c["blocks_per_mcu"] == 8 for c in whole)
    batch = [c["jpeg"] for c in med]
    _check_invert(tj, batch, "medium")
    pow2 = [c["jpeg"] for c in med if c["blocks_per_mcu"] in (4, 8)]
    assert len(pow2) == 3
    pow2 += [_standard("noise", 8, 96, 128, J.TJSAMP_422, 95), _standard("noise", 9, 100, 100, J.TJSAMP_GRAY, 95)]
    _check_invert(tj, pow2, "medium pow2")
    for j in (batch[1], batch[5]):
        assert np.array_equal(tj.decode(j), want_pixels(j))


def test_filters_on_general_layouts(tj, cases):
    """One table filter and one chain between the decode of a general layout and the encode:
    oracle decode -> numpy reference -> oracle encode, whole byte strings (the recipe of
    tests/test_gpu_lut_jpeg.py and test_gpu_chain_jpeg.py)."""
    import _chain_ref as CR
    from _chain_build import to_chain
    from vfilter import tables
    by = {c["file"]: c["jpeg"] for c in cases}
    picks = [by["small_112111_noise_40x71.jpg"], by["small_421111_noise_40x71.jpg"], by["small_221221_scene_17x13.jpg"]]
    perm = [np.random.default_rng(s).permutation(256).astype(np.uint8) for s in (31, 32, 33)]
    t3 = tables.stack(*perm)
    prog = CR.program_set("constant", 3)["edges"]
    for out_ss in (J.TJSAMP_422, J.TJSAMP_420):
        for j in picks:
            px = want_pixels(j)
            lut_ref = np.stack([perm[c][px[..., c]] for c in range(3)], axis=-1)
            assert tj.lut(j, t3, jpeg_subsample=out_ss) == J.encode(lut_ref, 85, J.TJPF_BGR, out_ss)
            assert tj.chain(j, to_chain(prog), jpeg_subsample=out_ss) == J.encode(CR.run(px, prog), 85, J.TJPF_BGR,
                                                                                 out_ss)
    got = tj.lut_batch(picks, t3)
    for g, j in zip(got, picks):
        px = want_pixels(j)
        assert g == J.encode(np.stack([perm[c][px[..., c]] for c in range(3)], axis=-1), 85, J.TJPF_BGR, J.TJSAMP_422)


def test_refused_streams_raise(tj, cases):
    """RGB-space streams (named as such in the error), layouts over 10 blocks per MCU and
    fractional ones: VFilterError from decode, invert, a batch and the asynchronous submit, all
    from the host parse; the context then decodes a good frame."""
    by = {c["file"]: c["jpeg"] for c in cases}
    good = by["small_222111_noise_40x71.jpg"]
    rgb = [c["jpeg"] for c in cases if c["colorspace"] == "rgb"]
    assert len(rgb) == 3
    rgb.append(S.with_ids(by["space_ycc_no_marker_ids_012.jpg"], b"RGB"))
    layouts = [S.with_factors(good, f) for f in S.OVER_10_BLOCKS + S.FRACTIONAL]
    for bad, match in [(b, "RGB") for b in rgb] + [(b, "sampling") for b in layouts]:
        for call in (tj.decode, tj.invert, lambda b: tj.decode_batch([good, b]), lambda b: tj.invert_batch([good, b, good]),
                     lambda b: tj.invert_batch_submit([good, b])):
            with pytest.raises(VFilterError, match=match):
                call(bad)
        with pytest.raises(ValueError):
            J.decode(bad)  # the oracle refuses them too
    assert np.array_equal(tj.decode(good), want_pixels(good))
    assert bytes(tj.invert(good)) == want_invert(good)


def test_colour_space_by_rule_gray_sampling_and_remuxed_headers(tj, cases, golden_dir):
    """Streams only libjpeg's rule identifies as YCbCr (Adobe transform 1 without JFIF; JFIF with
    ids R, G, B; JFIF and Adobe transform 0; no marker with ids 0,1,2 / Y,C,c / r,g,b), a gray
    frame whose SOF sampling byte is 0x22, 0x41, 0x33 or 0x14, and a 4:2:2 DRI stream with its
    header rewritten five ways (_jpeg_sampling.remuxes): libjpeg-turbo's hashes, and the fused
    invert against the oracle, alone and in one batch."""
    space = [c for c in _group(cases, "space") if c["colorspace"] != "rgb"]
    assert len(space) == 11
    for c in space:
        assert _sha(tj.decode(c["jpeg"])) == c["decoded_sha256"], c["file"]
    d = os.path.join(golden_dir, "jpeg")
    base = {c["file"]: c for c in json.load(open(os.path.join(d, "manifest.json")))["cases"]}[S.REMUX_BASE]
    jpg = open(os.path.join(d, S.REMUX_BASE), "rb").read()
    muxes = [m for _, m in S.remuxes(jpg)]
    for m in muxes:
        assert _sha(tj.decode(m)) == base["decoded_sha256"]
        assert _sha(bytes(tj.invert(m))) == base["inverted_sha256"]
        assert tj.decode_header(m)[:3] == (9, 33, J.TJSAMP_422)
    _check_invert(tj, [c["jpeg"] for c in space] + muxes, "rule and remux")
