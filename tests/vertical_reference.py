"""The cost volume with a vertical search (include/mccnn.h: mccnn_cost_volume_vertical_hwd), restated in NumPy.

    P(k; d,h,w)  = float32 sum of the 64 rounded products fl[h,w,:] * fr[h+k,w-d,:] (np.sum over the channel axis)
    S_L(d,h,w)   = max over k = -r..r, 0 <= h+k < H, of P(k; d,h,w)               w >= d
    S_R(d,h,w)   = max over k = -r..r, 0 <= h-k < H, of P(k; d,h-k,w+d)           w + d < W

with the maximum taken candidate by candidate in ascending k (best = s if (s > best or isnan(s)) else best, starting from
the first candidate), then the reference's border recurrences in float32 and the negation.  r = 0 is the oracle's
compute_cost_volume bit for bit (tests/test_vertical_cpu.py)."""
import numpy as np

_THREE = np.float32(3.)


def _take(best, seen, rows, s):
    """The definition's update of best[rows] with the candidate scores s (rows: a slice of image rows)."""
    b = best[rows]
    with np.errstate(invalid="ignore"):
        later = np.where((s > b) | np.isnan(s), s, b)
    best[rows] = np.where(seen[rows][:, None], later, s)
    seen[rows] = True


def _mean3(x1, x2, x3):
    """np.mean of three float32 values along an axis: the sum from the identity, in order, divided by 3."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.float32(0.) + x1
        s = s + x2
        s = s + x3
        return (s / _THREE).astype(np.float32)


def scores(fl, fr, ndisp, vertical_range):
    """(S_L, S_R) [D,H,W] float32 where they are defined (w >= d; w + d < W), zero elsewhere."""
    fl, fr = np.ascontiguousarray(fl, np.float32), np.ascontiguousarray(fr, np.float32)
    H, W, C = fl.shape
    D, r = int(ndisp), int(vertical_range)
    assert fr.shape == fl.shape and 0 <= r and 1 <= D <= W - 2
    sl, sr = np.zeros((D, H, W), np.float32), np.zeros((D, H, W), np.float32)
    for d in range(D):
        best_l, best_r = np.zeros((H, W - d), np.float32), np.zeros((H, W - d), np.float32)
        seen_l, seen_r = np.zeros(H, bool), np.zeros(H, bool)
        for k in range(-r, r + 1):
            lo, hi = max(0, -k), min(H, H - k)          # left rows h with 0 <= h + k < H
            if lo >= hi:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.sum(np.ascontiguousarray(fl[lo:hi, d:] * fr[lo + k:hi + k, :W - d]), axis=-1, dtype=np.float32)
            # P(k; d, h, w) at p[h - lo, w - d]: left pixel (h, w), and right pixel (h + k, w - d)
            _take(best_l, seen_l, slice(lo, hi), p)
            _take(best_r, seen_r, slice(lo + k, hi + k), p)
        assert seen_l.all() and seen_r.all()            # k = 0 serves every row
        sl[d, :, d:] = best_l
        sr[d, :, :W - d] = best_r
    return sl, sr


def fill_and_negate(sl, sr):
    """The border recurrences on the score volumes (left: column d - 1 downwards from the three columns to its right;
    right: column W - d upwards from the three to its left), then cost = -1 * score.  New arrays."""
    sl, sr = sl.copy(), sr.copy()
    D, H, W = sl.shape
    for d in range(D - 1, 0, -1):
        sl[d:, :, d - 1] = _mean3(sl[d:, :, d], sl[d:, :, d + 1], sl[d:, :, d + 2])
    for d in range(D - 1, 0, -1):
        sr[d:, :, W - d] = _mean3(sr[d:, :, W - d - 3], sr[d:, :, W - d - 2], sr[d:, :, W - d - 1])
    return (np.float32(-1.) * sl).astype(np.float32), (np.float32(-1.) * sr).astype(np.float32)


def compute_cost_volume_vertical(fl, fr, ndisp, vertical_range):
    """(lcv, rcv) [D,H,W] float32 of the definition."""
    return fill_and_negate(*scores(fl, fr, ndisp, vertical_range))


def hwd_to_dhw(vol_hwd, ndisp):
    """A pixel-major volume [H,W,Dp] -> [D,H,W] (the pad lanes dropped)."""
    return np.ascontiguousarray(np.transpose(np.asarray(vol_hwd)[:, :, :int(ndisp)], (2, 0, 1)))


def shift_rows(image, dy):
    """The image moved down by dy rows (up for dy < 0), its edge row repeated: row h holds row clip(h - dy)."""
    image = np.asarray(image)
    H = image.shape[0]
    return np.ascontiguousarray(image[np.clip(np.arange(H) - int(dy), 0, H - 1)])


def within_1px(disparity, truth, margin=4):
    """Share of pixels within 1 px of the truth, `margin` top and bottom rows left out."""
    err = np.abs(np.asarray(disparity, np.float64) - np.asarray(truth, np.float64))
    return float((err[margin:err.shape[0] - margin] <= 1.0).mean())
