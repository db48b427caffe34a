"""NumPy float64 references for the two tolerance-bounded kernels behind `--fast` and `--fast --separable-cbca`, and the
inputs their tests share.  Nothing here touches a GPU; tests/test_fast_kernels_reference_cpu.py checks this file against
the CPU oracle.

  scores64          the feature dot products of the cost volume (w >= d), in float64
  feature_families  named (fl, fr) pairs: the regimes in which a float32 accumulation chain rounds differently
  region_mean64     the cross-based region mean, summed directly (no prefix differences), in float64
  region_spans      the longest horizontal span and the vertical span of every region
  stream_model64    cbca_stream_kernel's stated algorithm (float64 prefixes, differences, stored reciprocal)
  cbca_image / cbca_volumes   the smooth image and the three volumes of the separable-aggregation tests
  separable_tolerance / tile_kernel_bound   the two per-voxel bounds those tests assert
"""
import glob
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = 64


# ---- cost volume ---------------------------------------------------------------------------------------------------------
def scores64(fl, fr, D):
    """-(fl[h,w,:] . fr[h,w-d,:]) in float64 for w >= d.  Returns (left, right, mask_left, mask_right), all [D,H,W]:
    left[d,h,w] is the score of (w, d), right[d,h,x] the score of (x + d, d); the masks mark the scored entries
    (w >= d; x < W - d), every other entry is 0."""
    fl64, fr64 = np.asarray(fl, np.float32).astype(np.float64), np.asarray(fr, np.float32).astype(np.float64)
    H, W, _ = fl64.shape
    left, right = np.zeros((D, H, W)), np.zeros((D, H, W))
    ml, mr = np.zeros((D, H, W), bool), np.zeros((D, H, W), bool)
    for d in range(min(D, W)):
        s = -(fl64[:, d:, :] * fr64[:, :W - d, :]).sum(-1)
        left[d, :, d:] = s
        right[d, :, :W - d] = s
        ml[d, :, d:] = True
        mr[d, :, :W - d] = True
    return left, right, ml, mr


def _unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.sqrt((a * a).sum(-1, keepdims=True))).astype(np.float32)


def _shifted(fl, d0, filler):
    """fr[h, x] = fl[h, x + d0]; the last d0 columns have no partner and take `filler`."""
    fr = filler.copy()
    W = fl.shape[1]
    fr[:, :W - d0] = fl[:, d0:]
    return fr


def _golden_rows():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN_DIR, "ref_*.npz"))):
        with np.load(p) as g:
            out.append((g["fl"].astype(np.float32), g["fr"].astype(np.float32)))
    assert out, "golden vectors missing"
    return out


EXACT_FAMILIES = ("onehot", "eighths")


def feature_families(H, W, seed):
    """{name: (fl, fr)}: float32 [H,W,64], |x| <= 1, unit norm to float32 rounding.  The matched families put a true match
    (score -1 up to rounding) on one diagonal of every row; the scores of the two EXACT_FAMILIES are exactly
    representable and any correct evaluation returns them exactly."""
    rng = np.random.default_rng(seed)
    g = _unit(rng.standard_normal((H, W, C)))
    other = _unit(rng.standard_normal((H, W, C)))
    fam = {"gauss": (g, other)}
    for d0 in (0, 3):
        fam["matched_%d" % d0] = (g, _shifted(g, min(d0, W - 1), other))
    fam["antiparallel"] = (g, -g)
    fam["near"] = (g, _unit(g.astype(np.float64) + 0.05 * rng.standard_normal((H, W, C))))
    nn = _unit(np.maximum(rng.standard_normal((H, W, C)), 0) + 1e-3)
    fam["nonneg"] = (nn, nn.copy())
    k = rng.permuted(np.tile(np.arange(C), (H, W, 1)), axis=-1)
    wide = _unit(rng.choice([-1.0, 1.0], (H, W, C)) * 2.0 ** (-k / 2.5))
    fam["wide"] = (wide, wide.copy())
    # the committed golden features (a trained network's), their rows laid side by side up to W
    rows = _golden_rows()
    gl, gr = np.empty((H, W, C), np.float32), np.empty((H, W, C), np.float32)
    for h in range(H):
        x, i = 0, h
        while x < W:
            a, b = rows[i % len(rows)]
            r = (h + i) % a.shape[0]
            n = min(a.shape[1], W - x)
            gl[h, x:x + n], gr[h, x:x + n] = a[r, :n], b[r, :n]
            x, i = x + n, i + 1
    fam["golden"] = (gl, gr)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    one_l, one_r = np.zeros((H, W, C), np.float32), np.zeros((H, W, C), np.float32)
    np.put_along_axis(one_l, ((3 * ww + 5 * hh) % C)[..., None], np.where(ww % 2, -1.0, 1.0)[..., None].astype(np.float32), -1)
    np.put_along_axis(one_r, ((5 * ww + 3 * hh) % C)[..., None],
                      np.where((ww >> 1) % 2, -1.0, 1.0)[..., None].astype(np.float32), -1)
    fam["onehot"] = (one_l, one_r)
    fam["eighths"] = tuple((rng.choice([-0.125, 0.125], (H, W, C))).astype(np.float32) for _ in range(2))
    return fam


def with_nans(fl, fr, seed, fraction=0.05):
    """Copies of (fl, fr) with a NaN in one channel of about `fraction` of the pixels of each view (no inf)."""
    rng = np.random.default_rng(seed)
    out = []
    for f in (fl, fr):
        f = f.copy()
        H, W, _ = f.shape
        hit = rng.random((H, W)) < fraction
        hit[0, W // 2] = True
        ch = rng.integers(0, C, (H, W))
        hs, ws = np.nonzero(hit)
        f[hs, ws, ch[hs, ws]] = np.nan
        out.append(f)
    return tuple(out)


# ---- cross-based aggregation -----------------------------------------------------------------------------------------
def _arm_planes(arms):
    a = np.asarray(arms).astype(np.int64)
    return a[..., 0], a[..., 1], a[..., 2], a[..., 3]          # up, down, left, right


def _hsum64(vol64, left, right):
    """hs[d,q,w] = sum of vol[d,q,w-left[q,w] .. w+right[q,w]], added term by term in float64."""
    W = vol64.shape[2]
    hs = vol64.copy()
    for dx in range(1, int(max(left.max(), right.max())) + 1):
        if dx >= W:
            break
        m = right[:, :W - dx] >= dx
        hs[:, :, :W - dx] += np.where(m, vol64[:, :, dx:], 0.0)
        m = left[:, dx:] >= dx
        hs[:, :, dx:] += np.where(m, vol64[:, :, :W - dx], 0.0)
    return hs


def _vsum64(hs, up, down):
    H = hs.shape[1]
    out = hs.copy()
    for dy in range(1, int(max(up.max(), down.max())) + 1):
        if dy >= H:
            break
        m = down[:H - dy, :] >= dy
        out[:, :H - dy, :] += np.where(m, hs[:, dy:, :], 0.0)
        m = up[dy:, :] >= dy
        out[:, dy:, :] += np.where(m, hs[:, :H - dy, :], 0.0)
    return out


def region_count(arms):
    up, down, left, right = _arm_planes(arms)
    return _vsum64((left + right + 1).astype(np.float64)[None], up, down)[0].astype(np.int64)


def region_sum64(vol, arms):
    """Float64 sum of the float32 values of every pixel's region: the vertical arm of the anchor is walked, and at each
    pixel on it that pixel's horizontal arm (pf:640-653).  Direct summation - no prefix sums, no cancellation: at most
    63 * 63 additions of error <= 2^-53 each, relative to the sum of the magnitudes."""
    up, down, left, right = _arm_planes(arms)
    vol64 = np.asarray(vol, np.float32).astype(np.float64)
    return _vsum64(_hsum64(vol64, left, right), up, down)


def region_mean64(vol, arms):
    return region_sum64(vol, arms) / region_count(arms).astype(np.float64)[None]


def region_spans(arms):
    """(n_h, n_v) [H,W]: the longest horizontal span left + right + 1 among the rows of the region, and up + down + 1."""
    up, down, left, right = _arm_planes(arms)
    span = left + right + 1
    H = span.shape[0]
    n_h = span.copy()
    for dy in range(1, int(max(up.max(), down.max())) + 1):
        if dy >= H:
            break
        n_h[:H - dy] = np.where(down[:H - dy] >= dy, np.maximum(n_h[:H - dy], span[dy:]), n_h[:H - dy])
        n_h[dy:] = np.where(up[dy:] >= dy, np.maximum(n_h[dy:], span[:H - dy]), n_h[dy:])
    return n_h, up + down + 1


def region_mean_naive(vol, arms, h, w):
    """One pixel of region_mean64, written as the definition reads (float64 [D])."""
    up, down, left, right = _arm_planes(arms)
    s, n = np.zeros(vol.shape[0]), 0
    for q in range(h - up[h, w], h + down[h, w] + 1):
        for x in range(w - left[q, w], w + right[q, w] + 1):
            s += vol[:, q, x].astype(np.float64)
            n += 1
    return s / n


STREAM_OUTW, STREAM_HL = 256, 15        # csrc/cross_cbca.hip, namespace s4: output columns of a strip, staged halo


def emit_reciprocal(count, up, down):
    """The float64 the streaming kernel multiplies by: 1/n with the vertical arms in its 12 low mantissa bits, the upper
    bits chosen so that the word as stored is nearest to 1/n (cross_count_kernel)."""
    rbits = (1.0 / count.astype(np.float64)).view(np.uint64)
    field = (down.astype(np.uint64) << np.uint64(7)) | ((31 - up).astype(np.uint64) << np.uint64(2))
    word = (((rbits - field + np.uint64(0x800)) >> np.uint64(12)) << np.uint64(12)) | field
    return word.view(np.float64)


def stream_model64(vol, arms):
    """cbca_stream_kernel as its comment states it, for arms <= 13: per 256-column strip a float64 inclusive row prefix
    that starts 15 columns left of the strip, horizontal-arm sums as prefix differences, their float64 running column
    prefix from the top row, vertical-arm sums as differences, times the stored reciprocal, rounded once to float32.
    (The kernel scans a row in another association and restarts the column prefix per row chunk: the same algorithm
    with roundings of the same size.  This model is here so that separable_tolerance() is checked without a GPU.)"""
    up, down, left, right = _arm_planes(arms)
    vol64 = np.asarray(vol, np.float32).astype(np.float64)
    D, H, W = vol64.shape
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    hs = np.empty_like(vol64)
    for w0 in range(0, W, STREAM_OUTW):
        s0, w1 = max(w0 - STREAM_HL, 0), min(w0 + STREAM_OUTW, W)
        s1 = min(w1 + 13, W)
        P = np.concatenate([np.zeros((D, H, 1)), np.cumsum(vol64[:, :, s0:s1], axis=2)], axis=2)   # P[i + 1]: through s0 + i
        cols = ww[:, w0:w1]
        hi = np.broadcast_to((cols + right[:, w0:w1] - s0 + 1)[None], (D, H, w1 - w0))
        lo = np.broadcast_to((cols - left[:, w0:w1] - s0)[None], (D, H, w1 - w0))
        hs[:, :, w0:w1] = np.take_along_axis(P, hi, 2) - np.take_along_axis(P, lo, 2)
    Q = np.concatenate([np.zeros((D, 1, W)), np.cumsum(hs, axis=1)], axis=1)
    above = np.take_along_axis(Q, np.broadcast_to((hh + down + 1)[None], (D, H, W)), 1)
    below = np.take_along_axis(Q, np.broadcast_to((hh - up)[None], (D, H, W)), 1)
    rn = emit_reciprocal(region_count(arms), up, down)
    return ((above - below) * rn[None]).astype(np.float32)


def ulp32(x):
    """The float32 spacing of the binade that holds the float64 value x (2^-149 below the normal range)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def separable_tolerance(mean64, max_abs_in):
    """Per voxel: half a float32 spacing of the exact mean (one rounding) plus 2^-34 max|in| for the float64 prefix
    arithmetic - column prefixes reach about 200 * 27 * max ~ 2^12.4 max, so an addition rounds by <= 2^-40.6 max, at most
    27 + 1 of them separate the two entries of a difference, and the stored reciprocal adds 2^-41 relative."""
    return 0.5 * ulp32(mean64) + 2.0 ** -34 * float(max_abs_in)


def tile_kernel_bound(vol, arms):
    """Per voxel bound for cbca_iter_kernel<R, TH, false> (distance 15 .. 32), the textbook one for sequential float32
    sums: (n_h + n_v + 2) 2^-24 (sum over the region of |v|) / n - n_h - 1 roundings in a row sum, n_v - 1 down the
    column, one in the division, three spare for the second-order terms."""
    n_h, n_v = region_spans(arms)
    mean_abs = region_sum64(np.abs(np.asarray(vol, np.float32)), arms) / region_count(arms)[None]
    return (n_h + n_v + 2)[None] * 2.0 ** -24 * mean_abs


CBCA_TAU = 0.02
CBCA_VOLUMES = ("unit", "sgm_scale", "mixed_scale")


def cbca_image(H, W, seed):
    """A smooth random image (uniform noise under a 9 x 9 box filter, zero padded, as
    test_full_size_cbca_streaming_vs_reference_order_cfg2 builds it) whose arms reach the limit in places and stop short
    in others, with a textured patch (raw noise) in one corner, where regions have size 1."""
    rng = np.random.default_rng(seed)
    raw = rng.random((H, W))
    pad = np.zeros((H + 8, W + 8))
    pad[4:-4, 4:-4] = raw
    box = np.zeros((H, W))
    for dy in range(9):
        for dx in range(9):
            box += pad[dy:dy + H, dx:dx + W]
    img = 0.3 * box / 81.0       # neighbours 9 and more columns apart differ by about 0.014: most arms pass CBCA_TAU, not all
    th, tw = max(H // 3, 1), max(W // 3, 1)
    img[:th, W - tw:] = raw[:th, W - tw:]
    return img.astype(np.float32)


def cbca_volumes(D, H, W, seed):
    """{name: float32 [D,H,W]}: uniform in [-1, 0]; SGM-scale, uniform in [-200, 0]; mixed scale, +-2^-e with e uniform
    in 0 .. 20."""
    rng = np.random.default_rng(seed)
    return {
        "unit": (-rng.random((D, H, W))).astype(np.float32),
        "sgm_scale": (-200.0 * rng.random((D, H, W))).astype(np.float32),
        "mixed_scale": (rng.choice([-1.0, 1.0], (D, H, W)) * 2.0 ** -rng.integers(0, 21, (D, H, W))).astype(np.float32),
    }


# (H, W, D) of the separable-aggregation tests at distance 14; D = None: 2 * compute units + 2, known on the device only
CBCA_STREAM_SHAPES = [
    (1, 40, 1), (2, 255, 3), (13, 256, 2), (14, 257, 3),      # strip edge either side, fewer rows than an arm
    (31, 513, 2), (33, 300, 5), (40, 33, 1),                  # ring wrap at 32 rows, batches of 3
    (130, 40, 3),                                             # two row chunks of 65, odd last plane group
    (200, 70, 2),                                             # three chunks
    (130, 40, None),                                          # whole rounds plus a chunked remainder
]
CBCA_TILE_CASES = [(L, shape) for L in (20, 32) for shape in ((40, 90, 3), (70, 140, 2))]


def cbca_case_seed(H, W, L):
    return (H * 1000 + W) * 100 + L


def nontrivial_region_floor(H, W, L):
    """What support_count.max() must exceed for the inputs to count as non-trivial: 200, or - in images too small to
    hold a region of 200 pixels - half of the largest region the image can hold."""
    return min(200, min(H, 2 * L - 1) * min(W, 2 * L - 1) // 2)
