"""A literal NumPy restatement of include/mccnn.h's confidence measures and of the sparsification score of
evaluation.py: per-pixel Python loops over np.float32 scalars, one IEEE operation per line, nothing vectorised.  It is the
reference of the confidence tests and shares no code with the library."""
import numpy as np

MSM, MMN, CUR, LRC = 1, 2, 4, 8
NAMES = ("msm", "mmn", "cur", "lrc")
BITS = dict(zip(NAMES, (MSM, MMN, CUR, LRC)))

_INF = np.float32(np.inf)
_NINF = np.float32(-np.inf)


def winner(c):
    """(d1, c1) of one pixel's costs: the first strict minimum from +inf; (-1, None) when nothing is below +inf."""
    best, d1 = _INF, -1
    for d in range(len(c)):
        if c[d] < best:
            best, d1 = c[d], d
    return d1, (c[d1] if d1 >= 0 else None)


def runner_up(c, d1):
    best = _INF
    for d in range(len(c)):
        if d != d1 and c[d] < best:
            best = c[d]
    return best


def pixel(c, w, right_row, measures):
    """(d1, the requested values of one pixel in ascending bit order).  c: its D float32 costs; right_row: row h of the
    right map (None unless LRC)."""
    D = len(c)
    k = bin(measures).count("1")
    d1, c1 = winner(c)
    if d1 == -1:
        return d1, [_NINF] * k
    out = []
    with np.errstate(all="ignore"):
        if measures & MSM:
            out.append(np.negative(c1))
        if measures & MMN:
            c2 = runner_up(c, d1)
            out.append(np.float32(c2 - c1))
        if measures & CUR:
            cm = c[d1 - 1] if d1 >= 1 else c[d1 + 1]
            cp = c[d1 + 1] if d1 <= D - 2 else c[d1 - 1]
            t = np.float32(np.float32(2.0) * c1)
            u = np.float32(cp - t)
            out.append(np.float32(u + cm))
        if measures & LRC:
            x = w - d1
            if x < 0:
                out.append(_NINF)
            else:
                r = right_row[x]
                if not (r >= np.float32(0.0)) or r == _INF:
                    out.append(_NINF)
                else:
                    out.append(np.negative(np.abs(np.float32(np.float32(d1) - r))))
    return d1, out


def confidence(vol_dhw, disp_right=None, measures=MSM | MMN | CUR | LRC):
    """vol_dhw [D,H,W] float32, disp_right [H,W] float32 -> planes [K,H,W] float32 and the winner map d1 [H,W] int."""
    vol = np.ascontiguousarray(vol_dhw, dtype=np.float32)
    D, H, W = vol.shape
    assert D >= 2 and 0 < measures < 16 and (disp_right is not None or not measures & LRC)
    k = bin(measures).count("1")
    out = np.empty((k, H, W), np.float32)
    d1s = np.empty((H, W), np.int64)
    hwd = np.ascontiguousarray(vol.transpose(1, 2, 0))
    for h in range(H):
        row = None if disp_right is None else [np.float32(v) for v in np.asarray(disp_right, np.float32)[h]]
        for w in range(W):
            c = [np.float32(v) for v in hwd[h, w]]
            d1s[h, w], vals = pixel(c, w, row, measures)
            for i in range(k):
                out[i, h, w] = vals[i]
    return out, d1s


def plane_index(measures, name):
    """Where `name`'s plane sits among the planes of `measures`."""
    bit = BITS[name]
    assert measures & bit
    return bin(measures & (bit - 1)).count("1")


# ---- sparsification ---------------------------------------------------------------------------------------------------
def sparsification(conf, bad, region):
    """conf [H,W] float32; bad, region [H,W] bool.  Returns dict(n, e, auc, auc_optimal): the pixels of `region` ordered
    by confidence descending (NaN as -inf; ties by ascending pixel index), B(k) the bad ones among the first k,
    auc = (1/n) sum_k B(k)/k, auc_optimal = (1/n) sum_{k=n-e+1..n} (k-(n-e))/k with e = B(n); float64.  n = 0: NaN."""
    conf = np.asarray(conf, np.float32).reshape(-1)
    bad = np.asarray(bad, bool).reshape(-1)
    region = np.asarray(region, bool).reshape(-1)
    idx = np.flatnonzero(region)
    n = int(idx.size)
    key = conf[idx].astype(np.float64)
    key[np.isnan(key)] = -np.inf
    order = np.argsort(-key, kind="stable")
    b = bad[idx][order]
    e = int(b.sum())
    terms, opt = [], []
    run = 0
    for k in range(1, n + 1):
        run += int(b[k - 1])
        terms.append(np.float64(run) / np.float64(k))
        if k > n - e:
            opt.append(np.float64(k - (n - e)) / np.float64(k))
    with np.errstate(all="ignore"):
        auc = np.float64(np.sum(np.asarray(terms, np.float64))) / np.float64(n)
        auc_optimal = np.float64(np.sum(np.asarray(opt, np.float64))) / np.float64(n)
    return dict(n=n, e=e, auc=float(auc), auc_optimal=float(auc_optimal))


# ---- test volumes -------------------------------------------------------------------------------------------------------
def _pixels(N, count):
    """`count` pixel indices spread over the image (they repeat where the image is smaller)."""
    return [(17 * j + 3) % N for j in range(count)]


def make_volume(H, W, D, kind, seed):
    """[D,H,W] float32.  kind "normal": random normal costs; "quant": four levels (ties everywhere; on odd columns the
    lowest level is zero, of either sign).  On top, at single pixels: d1 forced to 0, D-1, 255 and 256; the runner-up in
    the next 256-group and in d1's own lane; exact ties; zeros of both signs as winner and runner-up; -inf once and
    twice; all NaN, all +inf, NaN but one; and NaN, -inf and -0.0 scattered over the voxels."""
    rng = np.random.default_rng(seed)
    N = H * W
    if kind == "normal":
        v = rng.standard_normal((N, D)).astype(np.float32)
    else:
        levels = np.array([[-0.5, 0.0, 0.25, 1.0], [0.0, 0.5, 0.75, 1.5]], np.float32)
        pick = rng.integers(0, 4, (N, D))
        v = levels[(np.arange(N) % W % 2)[:, None], pick]
        v[(v == 0) & (rng.random((N, D)) < 0.5)] = np.float32(-0.0)
    # (-inf wins wherever it stands: kept to about a quarter of the pixels, so that finite winners remain at any D)
    for val, p in ((np.nan, 0.02), (-np.inf, min(0.02, 0.25 / D)), (-0.0, 0.02)):
        v[rng.random((N, D)) < p] = np.float32(val)
    edits = []
    edits.append({0: -50.0})
    edits.append({D - 1: -50.0})
    edits.append({0: -50.0, D - 1: -50.0})                          # tie: first index, margin 0
    edits.append({0: -np.inf})
    edits.append({D - 1: -np.inf, 0: -np.inf})                      # inf - inf
    edits.append("nan")
    edits.append("inf")
    edits.append("nan_but_last")
    if D >= 8:
        edits.append({"fill": 1.0, 2: 0.0, 6: -0.0, 7: 0.0})       # zero beats zero: the runner-up keeps ITS sign
        edits.append({"fill": 1.0, 2: -0.0, 5: 0.0, 6: -0.0})
        edits.append({"fill": 1.0, 1: 0.0, D - 2: 0.0, D - 1: -0.0})
        edits.append({"fill": 0.0, 3: -0.0})
        edits.append({"fill": -0.0, D - 1: 0.0})
        edits.append({4: -50.0, 5: -49.0})                          # runner-up in d1's lane
        edits.append({5: -50.0, 4: -49.0})
    if D > 255:
        edits.append({255: -50.0})
        edits.append({255: -50.0, 254: -50.0})
    if D > 256:
        edits.append({256: -50.0})
        edits.append({256: -50.0, 255: -49.0})
        edits.append({3: -50.0, 256: -49.0})                        # runner-up in the next 256-group
        edits.append({256: -50.0, 3: -49.0})
        edits.append({3: -50.0, 256: -50.0})
    if D > 266:
        edits.append({8: -50.0, 265: -49.0})                        # ... and there in d1's own lane
        edits.append({265: -50.0, 8: -50.0})
    for i, e in zip(_pixels(N, len(edits)), edits):
        if e == "nan":
            v[i] = np.nan
        elif e == "inf":
            v[i] = np.inf
        elif e == "nan_but_last":
            v[i] = np.nan
            v[i, D - 1] = 2.0
        else:
            if "fill" in e:
                v[i] = np.float32(e["fill"])
            for d, val in e.items():
                if d != "fill":
                    v[i, d] = np.float32(val)
    return np.ascontiguousarray(v.reshape(H, W, D).transpose(2, 0, 1))


def make_right_map(vol_dhw, seed):
    """A right map [H,W] for a left volume: mostly the left winner of the pixel it is read from or a neighbour of it,
    with fractions, and NaN, +-inf, -1, -0.0, other negatives and values >= D scattered over it."""
    rng = np.random.default_rng(seed)
    D, H, W = vol_dhw.shape
    with np.errstate(invalid="ignore"):
        d1 = np.argmin(np.where(np.isnan(vol_dhw), np.inf, vol_dhw), axis=0)
    r = np.zeros((H, W), np.float32)
    for h in range(H):
        for w in range(W):
            x = w - d1[h, w]
            if x >= 0:
                r[h, x] = d1[h, w]
    r += rng.integers(-1, 2, (H, W)).astype(np.float32)
    frac = rng.random((H, W)) < 0.2
    r[frac] += rng.random((H, W)).astype(np.float32)[frac]
    specials = [np.nan, np.inf, -np.inf, -1.0, -0.0, -0.25, -3.0, float(D), D + 0.5, 1.0e9]
    where = rng.random((H, W))
    for k, val in enumerate(specials):
        r[(where >= 0.03 * k) & (where < 0.03 * (k + 1))] = np.float32(val)
    return r


def to_hwd(vol_dhw, pad):
    """The pixel-major copy [H,W,Dp] of a [D,H,W] volume, its pad lanes filled with `pad`."""
    D, H, W = vol_dhw.shape
    Dp = (D + 3) & ~3
    out = np.full((H, W, Dp), np.float32(pad), np.float32)
    out[:, :, :D] = vol_dhw.transpose(1, 2, 0)
    return out
