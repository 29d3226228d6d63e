"""The numpy reference of the separable filter for the sep tests: ``_conv_ref.pad`` with the matching
mode, then the integer definition -- two 1-D passes in int64 (correlation, anchor at the centre), one
scaling at the end (none, a shift rounded half to even or half up, or an odd divisor to nearest),
saturate.  A transcription of the definition; shares no code with ``vfilter``."""
import numpy as np

from _conv_ref import pad


def accumulate(src, kx, ky, border="reflect101"):
    """acc[y, x, c] = sum_j ky[j] * sum_i kx[i] * src[by(y + j - kh//2), bx(x + i - kw//2), c], int64."""
    kx = np.asarray(kx, dtype=np.int64)
    ky = np.asarray(ky, dtype=np.int64)
    assert kx.ndim == 1 and ky.ndim == 1 and kx.size % 2 == 1 and ky.size % 2 == 1
    img = np.asarray(src)
    assert img.dtype == np.uint8
    flat = img.ndim == 2
    if flat:
        img = img[:, :, None]
    h, w, _ = img.shape
    p = pad(img.astype(np.int64), ky.size // 2, kx.size // 2, border)
    rows = np.zeros((p.shape[0], w, img.shape[2]), dtype=np.int64)  # the horizontal pass, on every padded row
    for i in range(kx.size):
        rows += kx[i] * p[:, i:i + w]
    acc = np.zeros(img.shape, dtype=np.int64)
    for j in range(ky.size):
        acc += ky[j] * rows[j:j + h]
    assert np.abs(acc).max(initial=0) < 2 ** 24
    return acc[:, :, 0] if flat else acc


def scale(acc, shift=0, divisor=1, rounding="half_even"):
    """The definition's q: acc, round(acc / 2^shift) or floor((2 acc + d) / (2 d))."""
    assert shift == 0 or divisor == 1
    if divisor != 1:
        assert divisor % 2 == 1
        return (2 * acc + divisor) // (2 * divisor)  # numpy's // floors
    if shift == 0:
        return acc
    if rounding == "half_up":
        return (acc + (1 << (shift - 1))) >> shift
    assert rounding == "half_even"
    f = acc >> shift  # arithmetic: floor
    r = acc & ((1 << shift) - 1)
    h = 1 << (shift - 1)
    return f + ((r > h) | ((r == h) & ((f & 1) == 1)))


def sep(src, kx, ky, shift=0, divisor=1, rounding="half_even", border="reflect101"):
    return np.clip(scale(accumulate(src, kx, ky, border), shift, divisor, rounding), 0, 255).astype(np.uint8)


def box(src, kw, kh, normalize=True, border="reflect101"):
    return sep(src, np.ones(kw, int), np.ones(kh, int), 0, kw * kh if normalize else 1, border=border)


def stats(src, kx, ky, shift, border="reflect101"):
    """(ties whose floor is even, ties whose floor is odd, negative accumulators, saturated outputs)."""
    acc = accumulate(src, kx, ky, border)
    q = scale(acc, shift)
    tie = (acc & ((1 << shift) - 1)) == (1 << (shift - 1)) if shift else np.zeros(acc.shape, bool)
    odd = ((acc >> shift) & 1) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum()), int((acc < 0).sum()), int(((q < 0) | (q > 255)).sum())


BINOMIAL9 = np.array([1, 8, 28, 56, 70, 56, 28, 8, 1])


def kernel_set():
    """The kernels the tests use, as name -> (kx, ky, shift)."""
    ends9 = np.zeros(9, dtype=np.int64)
    ends9[0] = ends9[8] = 1
    return {
        "ends9": (ends9, np.array([1]), 1),  # (a + b) / 2: half of all sums are ties
        "rand31x31": (np.random.default_rng(31).integers(-8, 9, 31), np.random.default_rng(32).integers(-8, 9, 31), 9),
        "rand15x5": (np.random.default_rng(15).integers(-20, 21, 15), np.random.default_rng(5).integers(-9, 10, 5), 7),
    }


def rand_taps(kw, kh):
    """Signed random taps of kw x kh, asymmetric on both axes (a flip or a swap of the axes cannot pass),
    with a shift that leaves the results in range."""
    rng = np.random.default_rng([21, kw, kh])
    kx, ky = rng.integers(-6, 10, kw), rng.integers(-6, 10, kh)
    if kw == 1:
        kx[0] = 3
    if kh == 1:
        ky[0] = 5
    total = int(np.abs(kx).sum() * np.abs(ky).sum())
    assert total <= 65536
    return kx, ky, max(0, min(16, total.bit_length() - 3))
