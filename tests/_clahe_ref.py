"""An independent numpy reference of CLAHE, written from the rule's definition: the
reflected extension, the tile histograms by ``np.bincount``, clip and redistribute in Python integers,
the table and the four-table blend in ``np.float32`` arithmetic -- every float operation is one numpy
operation on float32 values, so each is rounded on its own and nothing is promoted to double.
Nothing here is imported from ``vfilter``."""
import numpy as np

F = np.float32


def reflect101(p: int, n: int) -> int:
    """Where position ``p`` of an axis of ``n`` elements reads: gfedcb|abcdefgh|gfedcba, repeatedly."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def geometry(h: int, w: int, tiles_x: int, tiles_y: int):
    """``(He, We, th, tw)``: the extended frame and a tile."""
    if w % tiles_x == 0 and h % tiles_y == 0:
        he, we = h, w
    else:
        we, he = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    return he, we, he // tiles_y, we // tiles_x


def clip_of(clip_q8: int, area: int) -> int:
    return max((clip_q8 * area) >> 16, 1)


def redistribute(h, clip: int):
    """The bins after the clip (0: none) and the redistribution, as Python integers."""
    h = [int(v) for v in h]
    if clip > 0:
        excess = sum(max(v - clip, 0) for v in h)
        h = [min(v, clip) for v in h]
        batch = excess // 256
        residual = excess - 256 * batch
        h = [v + batch for v in h]
        if residual > 0:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:  # cv2's loop itself, not the closed form
                h[i] += 1
                i += step
                residual -= 1
    return h


def table(h, area: int, clip: int) -> np.ndarray:
    """A tile's table from its histogram ``h``; ``clip`` in counts, 0 for none."""
    cum = np.cumsum(np.array(redistribute(h, clip), np.int64))
    scale = F(255.0) / F(area)  # one float32 divide; F(int) rounds to nearest even
    r = np.rint(cum.astype(np.float32) * scale)  # int64 -> float32 to nearest even, one float32 multiply, half to even
    return np.clip(r, 0, 255).astype(np.uint8)


def weights(n: int, side: int, tiles: int, xs=None):
    """``(t1, t2, a, a1)`` for every coordinate of an axis of ``n`` frame elements (or for ``xs``)."""
    x = (np.arange(n, dtype=np.int64) if xs is None else np.asarray(xs, np.int64)).astype(np.float32)
    inv = F(1.0) / F(side)
    txf = x * inv - F(0.5)  # two float32 operations
    t = np.floor(txf)
    a = txf - t
    a1 = F(1.0) - a
    t = t.astype(np.int64)
    return np.maximum(t, 0), np.minimum(t + 1, tiles - 1), a, a1


def blend(t11, t12, t21, t22, xa, xa1, ya, ya1):
    """The pixel rule on float32 arrays or scalars: six products and three sums, each rounded."""
    t11, t12, t21, t22 = (np.asarray(v).astype(np.float32) for v in (t11, t12, t21, t22))
    res = (t11 * xa1 + t12 * xa) * ya1 + (t21 * xa1 + t22 * xa) * ya
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def tile_tables(plane: np.ndarray, clip_q8: int, tiles_x: int, tiles_y: int) -> np.ndarray:
    """``(tiles_y, tiles_x, 256)`` uint8: every tile's table of one ``H x W`` plane."""
    h, w = plane.shape
    he, we, th, tw = geometry(h, w, tiles_x, tiles_y)
    ys = [reflect101(p, h) for p in range(he)]
    xs = [reflect101(p, w) for p in range(we)]
    ext = plane[np.ix_(ys, xs)]
    area = tw * th
    assert area < 1 << 31
    clip = clip_of(clip_q8, area) if clip_q8 > 0 else 0
    out = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            out[ty, tx] = table(np.bincount(tile.ravel(), minlength=256), area, clip)
    return out


def clahe_plane(plane: np.ndarray, clip_q8: int, tiles_x: int, tiles_y: int) -> np.ndarray:
    h, w = plane.shape
    _, _, th, tw = geometry(h, w, tiles_x, tiles_y)
    tabs = tile_tables(plane, clip_q8, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = weights(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = weights(h, th, tiles_y)
    r1, r2, c1, c2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    return blend(tabs[r1, c1, plane], tabs[r1, c2, plane], tabs[r2, c1, plane], tabs[r2, c2, plane],
                 xa[None, :], xa1[None, :], ya[:, None], ya1[:, None])


def clahe(src: np.ndarray, clip_q8: int, tiles_x: int = 8, tiles_y: int = 8, mask: int = 0) -> np.ndarray:
    """The filter on a uint8 ``H x W`` or ``H x W x C`` frame; the empty frame comes back as it is."""
    if src.size == 0:
        return src.copy()
    a = src.reshape(src.shape[0], src.shape[1], -1)
    channels = a.shape[2]
    if mask == 0:
        mask = (1 << channels) - 1
    assert mask >> channels == 0
    out = a.copy()
    for c in range(channels):
        if mask >> c & 1:
            out[:, :, c] = clahe_plane(np.ascontiguousarray(a[:, :, c]), clip_q8, tiles_x, tiles_y)
    return out.reshape(src.shape)
