"""The row-offset measurement and the cost volume along an offset (include/mccnn.h: mccnn_vertical_profile,
mccnn_vertical_offset_select, mccnn_cost_volume_offset_hwd), restated in NumPy.

P(k; d,h,w) and the maximum rule are those of tests/vertical_reference.py.  With k0 = clip(offset, -8, 8), r = range:

    S_L(d,h,w) = max over k = k0-r .. k0+r, 0 <= h+k < H, of P(k; d,h,w);      no such k: P(clip(k0, -h, H-1-h); d,h,w)
    S_R(d,h,w) = max over k = k0-r .. k0+r, 0 <= h-k < H, of P(k; d,h-k,w+d);  no such k: k = clip(k0, h-(H-1), h)

    b(k)[h,w]  = max over d = 0 .. min(D-1, w), ascending, of P(k; d,h,w)       profiled rows h = step//2 + i*step < H
    a pixel votes for the k of its largest b (candidates 0, -1, +1, -2, +2, ..., replaced only by a strictly greater
    one) unless one of its b(k) is NaN; votes[i][w // 64][k + R] counts them; the offset is the k of the largest total
    by the same order and rule."""
import numpy as np

import vertical_reference as vr

OFFSET_MAX = 8


def candidate_order(max_offset):
    """0, -1, +1, -2, +2, ..., -R, +R."""
    out = [0]
    for a in range(1, int(max_offset) + 1):
        out += [-a, a]
    return out


def _products(fl, fr, lo, hi, k, d):
    """P(k; d,h,w) for left rows lo <= h < hi at [h - lo, w - d]."""
    W = fl.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sum(np.ascontiguousarray(fl[lo:hi, d:] * fr[lo + k:hi + k, :W - d]), axis=-1, dtype=np.float32)


def offset_scores(fl, fr, ndisp, row_offset, vertical_range):
    """(S_L, S_R) [D,H,W] float32 where they are defined (w >= d; w + d < W), zero elsewhere."""
    fl, fr = np.ascontiguousarray(fl, np.float32), np.ascontiguousarray(fr, np.float32)
    H, W, _ = fl.shape
    D, r = int(ndisp), int(vertical_range)
    k0 = min(max(int(row_offset), -OFFSET_MAX), OFFSET_MAX)
    assert fr.shape == fl.shape and 0 <= r and 1 <= D <= W - 2
    sl, sr = np.zeros((D, H, W), np.float32), np.zeros((D, H, W), np.float32)
    for d in range(D):
        best_l, best_r = np.zeros((H, W - d), np.float32), np.zeros((H, W - d), np.float32)
        seen_l, seen_r = np.zeros(H, bool), np.zeros(H, bool)
        for k in range(k0 - r, k0 + r + 1):
            lo, hi = max(0, -k), min(H, H - k)          # left rows h with 0 <= h + k < H
            if lo >= hi:
                continue
            p = _products(fl, fr, lo, hi, k, d)
            vr._take(best_l, seen_l, slice(lo, hi), p)
            vr._take(best_r, seen_r, slice(lo + k, hi + k), p)
        for h in np.flatnonzero(~seen_l):               # no candidate row inside the image: the nearest image row
            kc = min(max(k0, -h), H - 1 - h)
            best_l[h] = _products(fl, fr, h, h + 1, kc, d)[0]
        for h in np.flatnonzero(~seen_r):               # right row h against left row h - kc
            kc = min(max(k0, h - (H - 1)), h)
            best_r[h] = _products(fl, fr, h - kc, h - kc + 1, kc, d)[0]
        sl[d, :, d:] = best_l
        sr[d, :, :W - d] = best_r
    return sl, sr


def compute_cost_volume_offset(fl, fr, ndisp, row_offset, vertical_range):
    """(lcv, rcv) [D,H,W] float32 of the definition."""
    return vr.fill_and_negate(*offset_scores(fl, fr, ndisp, row_offset, vertical_range))


def profile_rows(H, row_step):
    return len(range(int(row_step) // 2, int(H), int(row_step)))


def best_scores(fl, fr, ndisp, h, k):
    """b(k)[w] of row h: the maximum over d = 0 .. min(D-1, w), d ascending, NaN sticky."""
    W = fl.shape[1]
    b = np.zeros(W, np.float32)
    for d in range(int(ndisp)):
        p = _products(fl, fr, h, h + 1, k, d)[0]
        if d == 0:
            b[:] = p
        else:
            with np.errstate(invalid="ignore"):
                b[d:] = np.where((p > b[d:]) | np.isnan(p), p, b[d:])
    return b


def vertical_profile(fl, fr, ndisp, max_offset, row_step):
    """votes uint32 [n_rows, ceil(W / 64), 2R + 1]."""
    fl, fr = np.ascontiguousarray(fl, np.float32), np.ascontiguousarray(fr, np.float32)
    H, W, _ = fl.shape
    R, step = int(max_offset), int(row_step)
    assert 0 <= R <= OFFSET_MAX and step >= 1
    rows = range(step // 2, H, step)
    votes = np.zeros((len(rows), (W + 63) // 64, 2 * R + 1), np.uint32)
    for i, h in enumerate(rows):
        b = {k: best_scores(fl, fr, ndisp, h, k) for k in range(-R, R + 1) if 0 <= h + k < H}
        nan = np.zeros(W, bool)
        for v in b.values():
            nan |= np.isnan(v)
        best, winner = b[0].copy(), np.zeros(W, np.int64)
        for k in candidate_order(R)[1:]:
            if k in b:
                with np.errstate(invalid="ignore"):
                    better = b[k] > best
                best[better], winner[better] = b[k][better], k
        for w in np.flatnonzero(~nan):
            votes[i, w // 64, winner[w] + R] += 1
    return votes


def offset_select(votes, max_offset):
    """(offset, totals uint64 [2R + 1])."""
    R = int(max_offset)
    totals = np.asarray(votes, np.uint64).reshape(-1, 2 * R + 1).sum(axis=0, dtype=np.uint64)
    best, offset = totals[R], 0
    for k in candidate_order(R)[1:]:
        if totals[k + R] > best:
            best, offset = totals[k + R], k
    return int(offset), totals


def share(totals, offset, max_offset):
    """The winner's share of all votes (0.0 without votes)."""
    n = int(np.asarray(totals, np.uint64).sum())
    return float(int(totals[int(offset) + int(max_offset)])) / n if n else 0.0
