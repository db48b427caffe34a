"""Shared by the ingest tests: the seeded uint8 images, NumPy's own standardisation (the reference of every check) and a
plain-Python statement of NumPy's summation order S, kept apart from the kernel's (csrc/ingest.hip)."""
import numpy as np

CHUNK = 8192     # np.getbufsize(): the reduction is fed in pieces of this many elements
SHAPES = [(1, 7), (3, 5), (40, 64), (64, 128), (128, 256), (5, 1639), (8, 1029), (97, 1031), (500, 750), (375, 1242),
          (2000, 3000)]
HISTOGRAMS = {"uniform": (0, 255), "narrow_120_123": (120, 123), "narrow_200_255": (200, 255)}


def image_u8(shape, hist, C, seed):
    """Seeded uint8 image [H,W] (C = 1) or [H,W,C]: every byte uniform in the histogram's range (the alpha byte of
    C = 4 uniform in 0 .. 255: it must not matter)."""
    lo, hi = HISTOGRAMS[hist]
    rng = np.random.default_rng([seed, shape[0], shape[1], C, lo, hi])
    if C == 1:
        return rng.integers(lo, hi + 1, size=shape, dtype=np.uint8)
    img = rng.integers(lo, hi + 1, size=shape + (C,), dtype=np.uint8)
    if C == 4:
        img[:, :, 3] = rng.integers(0, 256, size=shape, dtype=np.uint8)
    return img


def gray_of(img):
    """util.read_gray's grey stage on a decoded array (util.py:107-116)."""
    if img.ndim == 2:
        return img
    rgb = img[:, :, :3].astype(np.uint32)
    return ((rgb[:, :, 0] * 9797 + rgb[:, :, 1] * 19234 + rgb[:, :, 2] * 3737) >> 15).astype(np.uint8)


def numpy_standardise(gray_u8):
    """match.py:214-219, NumPy's own evaluation: the reference."""
    g = gray_u8.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1))


def pairwise(c):
    """NumPy's pairwise routine P on a 1-D float32 array."""
    m = len(c)
    if m < 8:
        res = np.float32(0)
        for v in c:
            res = np.float32(res + v)
        return res
    if m <= 128:
        r = c[:8].copy()                       # eight accumulators; elementwise float32 adds
        i = 8
        while i < m - m % 8:
            r = r + c[i:i + 8]
            i += 8
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                         + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in c[i:]:
            res = np.float32(res + v)
        return res
    m2 = m // 2
    m2 -= m2 % 8
    return np.float32(pairwise(c[:m2]) + pairwise(c[m2:]))


def stated_sum(a):
    """S: chunks of 8192 of the flat C-order array, each summed by P, the chunk sums added left to right."""
    flat = np.ascontiguousarray(a, dtype=np.float32).ravel()
    s = np.float32(0)
    for k in range(0, len(flat), CHUNK):
        s = np.float32(s + pairwise(flat[k:k + CHUNK]))
    return s


def stated_standardise(gray_u8):
    """(mean, std, out) by the statement: float32 throughout."""
    g = gray_u8.astype(np.float32)
    n = np.float32(g.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float32(stated_sum(g) / n)
        x = g - mean
        std = np.sqrt(np.float32(stated_sum(x * x) / n))
        return mean, std, (g - mean) / std


def bits(a):
    """uint32 patterns with every NaN mapped to one pattern (NaNs compare as NaNs)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7fc00000
    return u
