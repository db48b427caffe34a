"""A literal NumPy reference for the last third of the path (a7-a11 of include/mccnn.h, which cites pf:239-470) and
for the region list of a3, kept with the tests.

Per-pixel Python loops that CALL NumPy for every reduction (np.median, np.sum, np.linalg.norm, float32 scalars), so
that the summation order, the NaN propagation and the signs of zeros are NumPy's own and not a second hand-written
guess.  Slow by design: a few thousand pixels per image at most.  Plain module, no fixtures.

Where the reference's behaviour is undefined the restatement says so and follows the header instead:
  * lr_status: a LEFT disparity <= -1 or NaN makes the reference index the right map out of bounds or raise;
    include/mccnn.h says mccnn_lr_status treats such a disparity as an occlusion - status 2, asserted, not excluded.
    (A value in (-1, 0) is defined: int() truncates it to 0.)
  * subpixel_enhance: int() of a NaN or an infinite disparity raises in the reference and the header gives it no
    meaning; this module raises too (callers keep such values out of sub-pixel INPUTS; -1, fractional values and
    values >= D are all defined and covered).
  * disparity_prediction: the reference asserts that some cost is below +inf; the header says such a pixel gets -1.
"""
import warnings

import numpy as np

F32 = np.float32


def _a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def disparity_prediction_one(volume):
    """First strict minimum over d, as float32; -1 where no cost is below +inf (header rule)."""
    vol = _a32(volume)
    D, H, W = vol.shape
    out = np.empty((H, W), dtype=np.float32)
    for h in range(H):
        for w in range(W):
            best, arg = float("inf"), -1
            for d in range(D):
                if vol[d, h, w] < best:
                    best, arg = vol[d, h, w], d
            out[h, w] = arg
    return out


def disparity_prediction(left_volume, right_volume):
    return disparity_prediction_one(left_volume), disparity_prediction_one(right_volume)


def lr_status(left_map, right_map, ndisp):
    """0 match, 1 mismatch, 2 occlusion."""
    dl, dr = _a32(left_map), _a32(right_map)
    H, W = dl.shape
    st = np.zeros((H, W), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for h in range(H):
            for w in range(W):
                lf = dl[h, w]
                if not (lf > -1):              # undefined in the reference; the header's contract: an occlusion
                    st[h, w] = 2
                    continue
                ld = int(lf)
                if w < ld:
                    st[h, w] = 2
                    continue
                if abs(ld - dr[h, w - ld]) <= 1:       # Python int - float32 scalar: float32 (NumPy 2)
                    continue
                for d in range(min(w + 1, ndisp)):
                    if abs(d - dr[h, w - d]) <= 1:
                        st[h, w] = 1
                        break
                if st[h, w] == 0:
                    st[h, w] = 2
    return st


def _first_match(values, status, positions):
    for q in positions:
        if status[q] == 0:
            return [values[q]]
    return []


def interpolate(left_map, status):
    """Status 1: np.median of the nearest status-0 values to the right, left, below, above (in that order); status 2:
    the nearest status-0 value to the right; the raw value where there is none, and for any other status word."""
    dl = _a32(left_map)
    H, W = dl.shape
    out = np.empty((H, W), dtype=np.float32)
    for h in range(H):
        for w in range(W):
            s = status[h, w]
            if s == 0:
                out[h, w] = dl[h, w]
            elif s == 1:
                nb = (_first_match(dl, status, [(h, x) for x in range(w + 1, W)])
                      + _first_match(dl, status, [(h, x) for x in range(w - 1, -1, -1)])
                      + _first_match(dl, status, [(y, w) for y in range(h + 1, H)])
                      + _first_match(dl, status, [(y, w) for y in range(h - 1, -1, -1)]))
                out[h, w] = np.median(np.array(nb, dtype=np.float32)) if nb else dl[h, w]
            elif s == 2:
                nb = _first_match(dl, status, [(h, x) for x in range(w + 1, W)])
                out[h, w] = nb[0] if nb else dl[h, w]
            else:                              # a word lr_status never writes: no match, and nothing to fill it from
                out[h, w] = dl[h, w]
    return out


def interpolation(left_map, right_map, ndisp):
    return interpolate(left_map, lr_status(left_map, right_map, ndisp))


def subpixel_enhance(left_map, left_volume):
    """d - (C+ - C-) / (2 (C+ - 2 C + C-)) in float32 (NumPy 2 keeps float32 scalars float32 beside Python floats);
    unchanged where int(d - 1) < 0 or int(d + 1) >= D.  int() truncates toward zero."""
    dl, vol = _a32(left_map), _a32(left_volume)
    D, H, W = vol.shape
    out = np.empty((H, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for h in range(H):
            for w in range(W):
                d = dl[h, w]
                if not np.isfinite(d):
                    raise ValueError("subpixel_enhance: a non-finite disparity has no defined result")
                if int(d - 1) < 0 or int(d + 1) >= D:
                    out[h, w] = d
                    continue
                c_m, c_p, c = vol[int(d - 1), h, w], vol[int(d + 1), h, w], vol[int(d), h, w]
                out[h, w] = d - (c_p - c_m) / (2. * (c_p - 2. * c + c_m))
    return out


def _window(h, w, H, W, fh, fw):
    rh, rw = (fh - 1) // 2, (fw - 1) // 2
    return max(0, h - rh), min(H, h + rh + 1), max(0, w - rw), min(W, w + rw + 1)


def median_filter(left_map, fh, fw):
    dl = _a32(left_map)
    H, W = dl.shape
    out = np.empty((H, W), dtype=np.float32)
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # np.median announces every NaN it propagates
        for h in range(H):
            for w in range(W):
                hs, he, ws, we = _window(h, w, H, W, fh, fw)
                out[h, w] = np.median(dl[hs:he, ws:we])
    return out


def bilateral_table(fh, fw, mean, std_dev):
    """The spatial kernel: a normal density of the tap's distance from the centre, float64 evaluation, float32
    storage."""
    c1 = 1. / (np.sqrt(2 * np.pi) * std_dev)
    c2 = -1. / (2 * std_dev * std_dev)
    ch, cw = (fh - 1) // 2, (fw - 1) // 2
    tab = np.zeros((fh, fw), dtype=np.float32)
    for i in range(fh):
        for j in range(fw):
            x = np.sqrt((i - ch) ** 2 + (j - cw) ** 2)
            tab[i, j] = c1 * np.exp(c2 * ((x - mean) ** 2))
    return tab


def bilateral_filter(image, left_map, fh, fw, mean, std_dev, blur_threshold):
    img = _a32(image)
    if img.ndim == 2:
        img = img[:, :, None]
    dl = _a32(left_map)
    H, W = dl.shape
    tab = bilateral_table(fh, fw, mean, std_dev)
    ch, cw = (fh - 1) // 2, (fw - 1) // 2
    out = np.empty((H, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for h in range(H):
            for w in range(W):
                hs, he, ws, we = _window(h, w, H, W, fh, fw)
                patch = dl[hs:he, ws:we]
                taps = tab[ch - (h - hs):ch + (he - h), cw - (w - ws):cw + (we - w)]
                assert taps.shape == patch.shape
                diff = np.linalg.norm(img[hs:he, ws:we] - img[h, w], axis=-1)
                gate = (diff < blur_threshold).astype(np.float32)
                weights = np.multiply(gate, taps)
                wsum = np.sum(weights)
                out[h, w] = np.sum(np.multiply(weights, patch)) / wsum
    return out


def region_list(arms, L):
    """arms: [H,W,4] = up, down, left, right.  -> int32 [H,W,(2L)^2,2]: (row, column) pairs in the order vertical arm
    (self, up.., down..) x horizontal arm of that row (self, left.., right..), padded with -1."""
    arms = np.asarray(arms).astype(int)
    H, W, _ = arms.shape
    out = np.full((H, W, (2 * L) ** 2, 2), -1, dtype=np.int32)
    for h in range(H):
        for w in range(W):
            up, down = arms[h, w, 0], arms[h, w, 1]
            members = []
            for q in [h] + [h - k for k in range(1, up + 1)] + [h + k for k in range(1, down + 1)]:
                left, right = arms[q, w, 2], arms[q, w, 3]
                for x in [w] + [w - k for k in range(1, left + 1)] + [w + k for k in range(1, right + 1)]:
                    members.append((q, x))
            out[h, w, :len(members)] = members
    return out


# ---- the inputs both edge-test files share ------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 4), (4, 4), (4, 5), (5, 4), (5, 5), (6, 6), (9, 11), (4, 300)]
WINDOWS = [(1, 1), (1, 3), (3, 1), (3, 3), (5, 5), (3, 7), (7, 3), (7, 7), (1, 49), (49, 1), (5, 9), (9, 5), (3, 15)]
VALUE_CLASSES = ("random", "halves", "special")
BILATERAL_SETTINGS = [(6.0, 2.0), (1.5, 0.3)]          # (sigma, threshold)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], dtype=np.float32)


def make_map(shape, kind, rng):
    """A disparity map of one value class: random / quantised to halves (ties in every window) / ~15 % specials."""
    H, W = shape
    if kind == "halves":
        return (rng.integers(0, 9, size=shape) / 2.0).astype(np.float32)
    m = (rng.random(shape, dtype=np.float32) * F32(20) - F32(2)).astype(np.float32)
    if kind == "special":
        hit = rng.random(shape) < 0.15
        m[hit] = rng.choice(SPECIALS, size=int(hit.sum()))
        # small maps too hold a -0.0 (the value np.median turns into +0.0) and a NaN
        flat = m.reshape(-1)
        flat[int(rng.integers(flat.size))] = F32(-0.0)
        if flat.size > 2:
            flat[int(rng.integers(flat.size))] = F32(np.nan)
    return m


def make_image(shape, kind, rng):
    img = rng.standard_normal(shape).astype(np.float32)
    if kind == "special":
        img.reshape(-1)[int(rng.integers(img.size))] = F32(np.nan)
    return img


LR_SHAPES = [(1, 1, 1), (5, 1, 2), (2, 5, 3), (1, 300, 40), (4, 70, 64)]    # (H, W, D)


def make_lr_maps(H, W, D, rng, match=0.5, special_left=True):
    """Left and right maps on which all three states occur where the shape allows it: a share `match` of the left
    pixels is made consistent with the right map, the rest is random; then the edge values go in - left: fractional,
    >= D, -0.0, -0.5 (and, special_left, the undefined ones the header routes to status 2: -1, NaN, -inf); right: -1, -2,
    -1.0000001, fractional, >= D, NaN, +inf."""
    dr = rng.integers(0, D, size=(H, W)).astype(np.float32)
    dl = rng.integers(0, D, size=(H, W)).astype(np.float32)
    for h in range(H):
        for w in range(W):
            if rng.random() < match:
                cands = [d for d in range(min(w + 1, D)) if abs(d - dr[h, w - d]) <= 1]
                if cands:
                    dl[h, w] = cands[int(rng.integers(len(cands)))]
    n = H * W
    right_vals = np.array([-1, -2, -1.0000001, 0.5, 1.5, D - 0.5, D, D + 3, np.nan, np.inf], dtype=np.float32)
    left_vals = [0.5, 1.5, D - 1.5, D - 0.5, D, D + 2, -0.0, -0.5]
    if special_left:
        left_vals += [-1.0, -3.0, np.nan, -np.inf]
    left_vals = np.array(left_vals, dtype=np.float32)
    if n >= 4:
        hit = rng.random((H, W)) < 0.12
        dr[hit] = rng.choice(right_vals, size=int(hit.sum()))
        hit = rng.random((H, W)) < 0.12
        dl[hit] = rng.choice(left_vals, size=int(hit.sum()))
    return dl, dr


def case_rng(*key):
    return np.random.default_rng([7] + [int(k) for k in key])


def median_cases(window_index):
    for si, shape in enumerate(SHAPES):
        for ki, kind in enumerate(VALUE_CLASSES):
            yield shape, kind, make_map(shape, kind, case_rng(1, si, window_index, ki))


def bilateral_cases(window_index):
    for si, shape in enumerate(SHAPES):
        for ki, kind in enumerate(VALUE_CLASSES):
            rng = case_rng(2, si, window_index, ki)
            yield shape, kind, make_image(shape, kind, rng), make_map(shape, kind, rng)


def lr_cases():
    for si, (H, W, D) in enumerate(LR_SHAPES):
        for mi, match in enumerate((0.03, 0.5, 0.97)):
            for special_left in (False, True):
                dl, dr = make_lr_maps(H, W, D, case_rng(3, si, mi, special_left), match, special_left)
                yield (H, W, D), match, special_left, dl, dr


def subpixel_cases():
    """Integer, fractional (x.5), -1 (mccnn_wta's 'no winner'), -0.0, D - 1.5, D - 1, >= D disparities."""
    for si, (H, W, D) in enumerate(LR_SHAPES + [(3, 9, 5), (2, 7, 7)]):
        rng = case_rng(4, si)
        vol = rng.standard_normal((D, H, W)).astype(np.float32)
        if H * W > 4:
            vol[:, 0, 0] = 1.0                              # a flat cost curve: 0 / 0
        d = rng.integers(0, D, size=(H, W)).astype(np.float32)
        hit = rng.random((H, W)) < 0.4
        vals = np.array([0.5, 1.5, D - 1.5, D - 1, D - 0.5, D, D + 4, -1, -0.0, -0.5, 1.25], dtype=np.float32)
        d[hit] = rng.choice(vals, size=int(hit.sum()))
        yield (H, W, D), d, vol


def wta_volumes():
    """D = 1, 2, 3, 5, 7 (a remainder after groups of four), ties, an all-NaN, an all-+inf and a NaN-first pixel."""
    for di, D in enumerate((1, 2, 3, 5, 7, 12)):
        for ni, (H, W) in enumerate(((1, 1), (15, 17), (16, 16), (1, 257))):
            rng = case_rng(5, di, ni)
            vol = (rng.integers(0, 4, size=(D, H, W)) / 2.0).astype(np.float32)        # ties everywhere
            flat = vol.reshape(D, -1)
            if H * W > 8:
                flat[:, 1] = np.nan
                flat[:, 2] = np.inf
                flat[0, 3] = np.nan                                    # NaN first: never the minimum
                flat[:, 4] = -np.inf                                   # first of equal minima
                flat[:, 5] = np.float32(-0.0)
                flat[D - 1, 5] = 0.0                                   # -0.0 < +0.0 is false: index 0
                flat[D - 1, 6] = -7                                    # the last disparity wins
            yield vol
