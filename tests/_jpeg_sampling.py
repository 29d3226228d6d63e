"""JPEG sampling layouts past TurboJPEG's five, colour-space markers and header re-muxes
(test infrastructure shared by tests/golden/make_jpeg_sampling_golden.py and the
test_*jpeg_sampling* modules).

A three-component baseline frame may give each component sampling factors 1..4 as long as
every factor divides its direction's maximum and one interleaved MCU holds at most 10 blocks
(libjpeg's D_MAX_BLOCKS_IN_MCU; T.81 B.2.3).  FACTOR_SETS lists (h0, v0, h1, v1, h2, v2) for
every block count 4..10, luma that is not the densest component, Cb and Cr sampled
differently, expansion by 3 and 4 in each direction, and frames mixing the h2v1 and h1v2 fancy
upsamplers.
"""
from typing import Iterator, List, Sequence, Tuple

FACTOR_SETS: List[Tuple[int, ...]] = [
    # 4 blocks: Y, Cb, Cb, Cr -- luma is the sparse component
    (1, 1, 2, 1, 1, 1), (1, 1, 1, 2, 1, 1),
    # 5
    (3, 1, 1, 1, 1, 1), (1, 3, 1, 1, 1, 1), (2, 1, 1, 1, 2, 1), (1, 2, 1, 1, 1, 2), (1, 1, 1, 1, 3, 1),
    # 6: 4:1:1 and its transpose; all components alike at h = 2
    (4, 1, 1, 1, 1, 1), (1, 4, 1, 1, 1, 1), (2, 1, 2, 1, 2, 1),
    # 7
    (2, 2, 2, 1, 1, 1), (2, 2, 1, 2, 1, 1), (4, 1, 2, 1, 1, 1), (3, 1, 3, 1, 1, 1),
    # 8: (2,2, 2,1, 1,2) and (2,2, 1,2, 2,1) mix h1v2-fancy and h2v1-fancy chroma in one frame
    (2, 2, 2, 1, 1, 2), (2, 2, 1, 2, 2, 1), (2, 2, 2, 1, 2, 1), (3, 2, 1, 1, 1, 1),
    # 9
    (1, 1, 2, 2, 2, 2), (2, 2, 1, 1, 2, 2), (2, 2, 2, 2, 1, 1),
    # 10
    (4, 2, 1, 1, 1, 1), (2, 4, 1, 1, 1, 1),
]
# the sets of the medium (several sync workgroups) fixtures; the third is written with DRI 3 and
# optimised tables
MEDIUM_SETS: List[Tuple[int, ...]] = [(1, 1, 2, 1, 1, 1), (2, 2, 2, 1, 2, 1), (2, 2, 1, 2, 2, 1), (4, 1, 1, 1, 1, 1),
                                      (2, 2, 2, 1, 1, 1), (4, 2, 1, 1, 1, 1)]
# refused by libjpeg: over 10 blocks per MCU (jdinput.c JERR_BAD_MCU_SIZE), and a factor that does
# not divide its direction's maximum (jdsample.c JERR_FRACTIONAL_SAMPLING)
OVER_10_BLOCKS: List[Tuple[int, ...]] = [(3, 3, 1, 1, 1, 1), (4, 2, 2, 1, 1, 1), (2, 2, 2, 2, 2, 2), (4, 4, 1, 1, 1, 1),
                                         (4, 4, 4, 4, 4, 4)]
FRACTIONAL: List[Tuple[int, ...]] = [(3, 1, 2, 1, 1, 1), (2, 3, 1, 2, 1, 1), (4, 1, 3, 1, 1, 1), (2, 2, 1, 1, 3, 1)]
# the tests/golden/jpeg/ stream (standard 4:2:2 with DRI 2) that remuxes() rewrites
REMUX_BASE = "scene_33x9_q85_422_dri2.jpg"


def blocks_per_mcu(f: Sequence[int]) -> int:
    return sum(f[2 * k] * f[2 * k + 1] for k in range(3))


def tjsamp_of(f: Sequence[int]) -> int:
    """What tjDecompressHeader3 reports (turbojpeg.c getSubsamp): a TJSAMP_* value when chroma is
    1 x 1 and luma one of the six TurboJPEG shapes, else -1."""
    if tuple(f[2:]) != (1, 1, 1, 1):
        return -1
    return {(1, 1): 0, (2, 1): 1, (2, 2): 2, (1, 2): 4, (4, 1): 5}.get((f[0], f[1]), -1)


def name_of(f: Sequence[int]) -> str:
    return "".join(str(v) for v in f)


def segments(jpeg: bytes) -> Iterator[Tuple[int, int, int]]:
    """(marker, start, end) of each header segment of a stream written without fill bytes, SOS
    included (its end is where the entropy-coded data starts)."""
    i = 2
    while i + 4 <= len(jpeg):
        assert jpeg[i] == 0xFF, i
        m, n = jpeg[i + 1], (jpeg[i + 2] << 8) | jpeg[i + 3]
        yield m, i, i + 2 + n
        if m == 0xDA:
            return
        i += 2 + n
    raise AssertionError("no SOS")


def _find(jpeg: bytes, marker: int) -> Tuple[int, int]:
    for m, a, b in segments(jpeg):
        if m == marker:
            return a, b
    raise AssertionError(f"no marker {marker:#x}")


def with_factors(jpeg: bytes, f: Sequence[int]) -> bytes:
    """The stream with its SOF0 sampling bytes replaced (the entropy data no longer fits the
    layout: for the refusal tests, whose streams must be turned down from the header alone)."""
    a, _ = _find(jpeg, 0xC0)
    out = bytearray(jpeg)
    nc = out[a + 9]
    for c in range(nc):
        out[a + 11 + 3 * c] = (f[2 * c] << 4) | f[2 * c + 1]
    return bytes(out)


def with_gray_sampling(jpeg: bytes, hv: int) -> bytes:
    """A one-component stream with the SOF sampling byte set to ``hv``: a non-interleaved scan
    has one block per MCU whatever the factors say (T.81 A.2.2), so the picture is unchanged."""
    a, _ = _find(jpeg, 0xC0)
    assert jpeg[a + 9] == 1
    out = bytearray(jpeg)
    out[a + 11] = hv
    return bytes(out)


def with_ids(jpeg: bytes, ids: Sequence[int]) -> bytes:
    """Component ids rewritten in SOF0 and SOS."""
    a, _ = _find(jpeg, 0xC0)
    s, _ = _find(jpeg, 0xDA)
    out = bytearray(jpeg)
    for c, v in enumerate(ids):
        out[a + 10 + 3 * c] = v
        out[s + 5 + 2 * c] = v
    return bytes(out)


def _seg(marker: int, body: bytes) -> bytes:
    n = len(body) + 2
    assert n <= 65535
    return bytes([0xFF, marker, n >> 8, n & 255]) + body


def _tables(body: bytes, dht: bool) -> List[bytes]:
    """The tables of one DQT / DHT segment body."""
    out, j = [], 0
    while j < len(body):
        n = 17 + sum(body[j + 1:j + 17]) if dht else 1 + (128 if body[j] >> 4 else 64)
        out.append(body[j:j + n])
        j += n
    return out


def remuxes(jpeg: bytes) -> List[Tuple[str, bytes]]:
    """Header rewrites of one stream (which must carry a DRI) that leave the picture alone: the
    entropy-coded bytes are kept, and the decode is the original's."""
    segs = list(segments(jpeg))
    scan = jpeg[segs[-1][2]:]
    by = {}
    for m, a, b in segs:
        by.setdefault(m, []).append(jpeg[a:b])
    assert len(by[0xDB]) >= 2 and len(by[0xC4]) >= 4 and 0xDD in by
    app0, sof, sos, dri = by[0xE0][0], by[0xC0][0], by[0xDA][0], by[0xDD][0]
    dqts = [t for s in by[0xDB] for t in _tables(s[4:], False)]
    dhts = [t for s in by[0xC4] for t in _tables(s[4:], True)]
    soi = jpeg[:2]
    # one DHT segment with every table (jdmarker.c get_dht loops over the segment), each DQT on
    # its own with the second one after the frame header, where T.81 B.2.4 allows it too
    merged = soi + app0 + _seg(0xDB, dqts[0]) + sof + _seg(0xC4, b"".join(dhts)) + dri + \
        b"".join(_seg(0xDB, t) for t in dqts[1:]) + sos + scan
    # and the reverse: one DQT segment, one table per DHT in another order, after the DRI
    one_dqt = soi + app0 + _seg(0xDB, b"".join(dqts)) + sof + dri + b"".join(_seg(0xC4, t) for t in dhts[::-1]) + \
        sos + scan
    dri_first = soi + app0 + dri + b"".join(by[0xDB]) + sof + b"".join(by[0xC4]) + sos + scan
    # the longest segment there is (length field 65535), its payload full of 0xFF and of bytes
    # that read as markers (SOS, SOF2, EOI) to a parser that scans instead of skipping by length
    junk = (b"Exif\x00\x00" + b"\xff\xda\x00\x0c\x03\xff\xc2\xff\xd9\xff\xff\xd8\xff\x00" * 4681)[:65533]
    assert len(junk) == 65533
    big_app = soi + app0 + _seg(0xE1, junk) + _seg(0xFE, b"a comment \xff\xc0 with a marker in it") + \
        jpeg[segs[0][2]:]
    # fill bytes: any number of 0xFF may precede a marker (T.81 B.1.1.2)
    fill = soi + app0
    for k, (m, a, b) in enumerate(segs[1:]):
        fill += b"\xff" * (1 + 3 * (k % 3) if m in (0xDB, 0xC0, 0xC4, 0xDA) else 0) + jpeg[a:b]
    fill += scan
    return [("dht_merged_dqt_split", merged), ("dqt_merged_dht_reordered", one_dqt), ("dri_before_sof", dri_first),
            ("app1_65533_and_com", big_app), ("fill_bytes", fill)]
