"""An independent numpy reference of the level filter: the histogram by
``np.bincount``, the two table rules written from their definition with ``np.float32`` arithmetic, and
``level(src, rule, mask, link, clips)``.  Nothing here is imported from ``vfilter``."""
import numpy as np

EQUALIZE, STRETCH = 0, 1


def hist(src: np.ndarray) -> np.ndarray:
    """``(channels, 256)`` uint32 counts of a uint8 ``H x W`` or ``H x W x C`` frame."""
    a = src.reshape(src.shape[0] * src.shape[1], -1) if src.ndim >= 2 else src.reshape(-1, 1)
    return np.stack([np.bincount(a[:, c], minlength=256) for c in range(a.shape[1])]).astype(np.uint32)


def equalize_table(h, total: int) -> np.ndarray:
    """cv2.equalizeHist's table of the histogram ``h`` (integers) with ``total`` entries."""
    h = [int(v) for v in h]
    i0 = next(v for v in range(256) if h[v] != 0)
    if h[i0] == total:
        return np.arange(256, dtype=np.uint8)
    scale = np.float32(255.0) / np.float32(total - h[i0])  # float32 / float32: one correctly rounded divide
    table = np.zeros(256, np.uint8)
    s = 0
    for v in range(i0 + 1, 256):
        s += h[v]
        r = np.rint(np.float32(s) * scale)  # np.float32(int): to nearest even; the product: one float32 multiply
        table[v] = min(max(int(r), 0), 255)
    return table


def stretch_table(h, total: int, clip_lo: int, clip_hi: int) -> np.ndarray:
    h = [int(v) for v in h]
    cut_lo, cut_hi = (total * clip_lo) >> 16, (total * clip_hi) >> 16
    lo = next(v for v in range(256) if sum(h[:v + 1]) > cut_lo)
    hi = next(v for v in range(255, -1, -1) if sum(h[v:]) > cut_hi)
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    table = np.zeros(256, np.uint8)
    for v in range(256):
        table[v] = 0 if v <= lo else 255 if v >= hi else (510 * (v - lo) + (hi - lo)) // (2 * (hi - lo))
    return table


def table(h, total: int, rule: int, clip_lo: int = 0, clip_hi: int = 0) -> np.ndarray:
    return equalize_table(h, total) if rule == EQUALIZE else stretch_table(h, total, clip_lo, clip_hi)


def level(src: np.ndarray, rule: int, mask: int = 0, link: int = 0, clips=(0, 0)) -> np.ndarray:
    """The filter on a uint8 ``H x W`` or ``H x W x C`` frame; the empty frame comes back as it is."""
    if src.size == 0:
        return src.copy()
    a = src.reshape(src.shape[0], src.shape[1], -1)
    channels = a.shape[2]
    if mask == 0:
        mask = (1 << channels) - 1
    assert mask >> channels == 0
    hs = hist(a).astype(np.int64)
    pixels = a.shape[0] * a.shape[1]
    masked = [c for c in range(channels) if mask >> c & 1]
    out = a.copy()
    if link:
        t = table(sum(hs[c] for c in masked), pixels * len(masked), rule, *clips)
    for c in masked:
        out[:, :, c] = (t if link else table(hs[c], pixels, rule, *clips))[a[:, :, c]]
    return out.reshape(src.shape)
