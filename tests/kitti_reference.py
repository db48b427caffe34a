"""NumPy restatements of the KITTI entry points, written from the definitions in include/mccnn.h - no code shared with
the kernels.

encode / decode                 the kit's 16-bit code (this project rounds half to even where the kit truncates)
interpolate_background_walk     the kit's interpolateBackground as its literal sequential walks: a run counter along every
                                row, then the extrapolation to the left and to the right, then first / last valid per column
interpolate_background_nearest  the same function as include/mccnn.h states it (nearest valid neighbours), pixel by pixel
evaluate                        the scorer, on the tree of tests/evaluation_reference.py
"""
import numpy as np

import evaluation_reference as ref

REGIONS = ref.REGIONS


def valid(d):
    """Finite and >= 0; -0.0 counts."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d >= np.float32(0))


def encode(disp):
    disp = np.asarray(disp, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(disp * np.float32(256.0))              # float32 product, round half to even
        assert v.dtype == np.float32
        code = np.clip(np.where(valid(disp), v, 1), 1, 65535).astype(np.uint16)
    return np.where(valid(disp), code, np.uint16(0)).astype(np.uint16)


def decode(code):
    """uint16 -> float32, 0 -> +inf (Middlebury's "unknown"); v / 256 is exact."""
    code = np.asarray(code, np.uint16)
    return np.where(code == 0, np.float32(np.inf), code.astype(np.float32) / np.float32(256.0)).astype(np.float32)


def _min_right_left(left, right):
    """R < L ? R : L on float32 values."""
    return right if right < left else left


def interpolate_background_walk(disp):
    """The kit's loops.  Works on bit patterns through a float32 copy, so untouched pixels keep their bits."""
    d = np.array(disp, np.float32, copy=True)
    H, W = d.shape
    is_valid = valid(d)                      # kept up to date below: a filled pixel holds a valid value

    def ok(v, u):
        return bool(is_valid[v, u])

    def fill(rows, cols, value):
        d[rows, cols] = value
        is_valid[rows, cols] = True

    for v in range(H):
        count = 0
        for u in range(W):
            if ok(v, u):
                if count >= 1:
                    u1, u2 = u - count, u - 1
                    if u1 > 0 and u2 < W - 1:                    # a run with a valid pixel on either side
                        fill(v, slice(u1, u2 + 1), _min_right_left(d[v, u1 - 1], d[v, u2 + 1]))
                count = 0
            else:
                count += 1
        for u in range(W):                                       # extrapolate to the left
            if ok(v, u):
                fill(v, slice(0, u), d[v, u])
                break
        for u in range(W - 1, -1, -1):                           # extrapolate to the right
            if ok(v, u):
                fill(v, slice(u + 1, W), d[v, u])
                break
    for u in range(W):
        for v in range(H):                                       # extrapolate to the top
            if ok(v, u):
                fill(slice(0, v), u, d[v, u])
                break
        for v in range(H - 1, -1, -1):                           # extrapolate to the bottom
            if ok(v, u):
                fill(slice(v + 1, H), u, d[v, u])
                break
    return d


def interpolate_background_nearest(disp):
    """include/mccnn.h (b), pixel by pixel."""
    src = np.asarray(disp, np.float32)
    H, W = src.shape
    ok = valid(src)
    rows = np.array(src, np.float32, copy=True)
    for v in range(H):
        idx = np.flatnonzero(ok[v])
        for u in np.flatnonzero(~ok[v]):
            left, right = idx[idx < u], idx[idx > u]
            if left.size and right.size:
                rows[v, u] = _min_right_left(src[v, left[-1]], src[v, right[0]])
            elif left.size:
                rows[v, u] = src[v, left[-1]]
            elif right.size:
                rows[v, u] = src[v, right[0]]
    out = np.array(rows, np.float32, copy=True)
    ok = valid(rows)
    for u in range(W):
        idx = np.flatnonzero(ok[:, u])
        if idx.size:
            out[:idx[0], u] = rows[idx[0], u]
            out[idx[-1] + 1:, u] = rows[idx[-1], u]
    return out


def evaluate(disp, gt_occ, gt_noc, thresholds, interpolate=False):
    """thresholds: (abs, rel) pairs -> the dict of evaluation_reference.evaluate."""
    disp = np.asarray(disp, np.float32)
    if interpolate:
        disp = interpolate_background_walk(disp)
    disp = disp.reshape(-1)
    occ = np.asarray(gt_occ, np.uint16).reshape(-1)
    noc = occ if gt_noc is None else np.asarray(gt_noc, np.uint16).reshape(-1)
    invalid = ~valid(disp)
    out = {}
    for name, code in (("all", occ), ("nonocc", noc)):
        reg = code != 0
        g = code.astype(np.float32) / np.float32(256.0)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(disp - g)
            assert err.dtype == np.float32
            a = err.astype(np.float64)
            q = a * a
            scored = reg & ~invalid
            n_bad = []
            for t_abs, t_rel in thresholds:
                rel = np.float32(t_rel) * g                      # float32 product, rounded on its own
                assert rel.dtype == np.float32
                n_bad.append(int(np.count_nonzero(scored & (err > np.float32(t_abs)) & (err > rel))))
        out[name] = dict(n_valid=int(np.count_nonzero(reg)), n_invalid=int(np.count_nonzero(reg & invalid)), n_bad=n_bad,
                         sum_abs=ref.tree_sum(np.where(scored, a, 0.0)), sum_sq=ref.tree_sum(np.where(scored, q, 0.0)))
    return out


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


INVALID_CODES = (np.nan, np.inf, -np.inf, -1.0)
SEAMS = (63, 64, 127, 128, 255, 256, 257, 511, 512, 1023, 1024, 1279, 1280, 2047, 2048)     # lanes 63/64, segment seams


def make_holes_map(H, W, seed, whole_rows=()):
    """A seeded map for the interpolation: values on a coarse grid (so that neighbours tie) with +0.0 and -0.0 among them,
    and invalid runs - random ones, runs that start or end on every wave and segment seam the width has, a leading and a
    trailing run, in the 2049 row a run of 1300 pixels - in mixed NaN, +-inf and -1.  whole_rows: rows made invalid
    entirely."""
    rng = np.random.default_rng(seed)
    d = (rng.integers(0, 6, (H, W)) * 0.5).astype(np.float32)
    d[rng.random((H, W)) < 0.1] = np.float32(-0.0)
    hole = np.zeros((H, W), bool)
    for v in range(H):
        for _ in range(max(1, W // 40)):                        # random runs, 1 .. 70 long
            a = int(rng.integers(0, W))
            hole[v, a:a + int(rng.integers(1, 71))] = True
        for k, s in enumerate(x for x in SEAMS if x < W):       # a run ending on / starting on the seam, by row
            n = int(rng.integers(1, 9))
            if (v + k) % 3 == 0:
                hole[v, max(0, s - n + 1):s + 1] = True         # ends on s
            elif (v + k) % 3 == 1:
                hole[v, s:s + n] = True                         # starts on s
            else:
                hole[v, s] = False                              # a lone valid pixel on the seam
        if v % 4 == 1:
            hole[v, :int(rng.integers(1, W + 1))] = True        # leading run
        if v % 4 == 2:
            hole[v, W - int(rng.integers(1, W + 1)):] = True    # trailing run
        if W == 2049 and v % 2 == 0:
            hole[v, 300:1600] = True                            # across five segments
            d[v, 299], d[v, 1600] = (2.5, 1.0) if v % 4 == 0 else (1.0, 2.5)
            hole[v, 299] = hole[v, 1600] = False
    for v in whole_rows:
        hole[v] = True
    codes = np.asarray(INVALID_CODES, np.float32)[rng.integers(0, len(INVALID_CODES), (H, W))]
    return np.where(hole, codes, d).astype(np.float32)


D1 = ((3.0, 0.05),)
THR8 = ((0.5, 0.0), (1.0, 0.0), (2.0, 0.0), (3.0, 0.0), (3.0, 0.05), (4.0, 0.1), (5.0, 0.0), (2.0, 0.5))


def make_score_case(H, W, seed, noc_follows_occ=False, holes=0.05):
    """(disp, gt_occ, gt_noc): ground truth with zeros, gt_noc a subset of gt_occ's pixels (with some values of its own
    unless noc_follows_occ), estimates with every invalid code, and - once there is room - errors placed exactly on 3,
    one ulp above 3, and exactly on / one ulp around 0.05 * g (g = 100 and g = 80, where float32(0.05) * g rounds to 5
    and 4)."""
    rng = np.random.default_rng(seed)
    n = H * W
    occ = rng.integers(1, 200 * 256, n).astype(np.uint16)
    occ[rng.random(n) < 0.3] = 0
    noc = occ.copy()
    noc[rng.random(n) < 0.2] = 0
    if not noc_follows_occ:
        other = (rng.random(n) < 0.05) & (noc != 0)
        noc[other] = rng.integers(1, 200 * 256, int(other.sum())).astype(np.uint16)
    g = occ.astype(np.float32) / np.float32(256)
    disp = np.abs(g + rng.normal(0.0, 2.5, n).astype(np.float32)).astype(np.float32)
    for value, p in ((np.nan, holes / 2), (np.inf, 0.01), (-np.inf, 0.01), (-1.0, holes / 2), (-0.0, 0.01)):
        disp[rng.random(n) < p] = value
    if n >= 16:
        pos = iter(rng.permutation(n)[:16])
        up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
        down = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
        for code, d in ((50 * 256, 53.0), (50 * 256, up(53.0)), (50 * 256, 47.0), (50 * 256, down(47.0)),   # |err| = 3, 3+
                        (100 * 256, 105.0), (100 * 256, up(105.0)), (100 * 256, down(105.0)),                # 0.05 g = 5
                        (80 * 256, 76.0), (80 * 256, down(76.0)), (80 * 256, up(76.0)),                      # 0.05 g = 4
                        (1, 0.0), (1, -0.0)):
            i = next(pos)
            occ[i] = noc[i] = code
            disp[i] = d
        for v in INVALID_CODES:
            i = next(pos)
            occ[i], noc[i], disp[i] = 7 * 256, 7 * 256, v
    return disp.reshape(H, W), occ.reshape(H, W), noc.reshape(H, W)


def encode_specials():
    """The values the issue names for the encode, with what they must give."""
    f = np.float32
    return [(f(0.0), 1), (f(-0.0), 1), (f(0.5 / 256), 1), (f(1.5 / 256), 2), (f(2.5 / 256), 2), (f(3.5 / 256), 4),
            (f(255.998), 65535), (f(256.0), 65535), (f(1e9), 65535), (f(3e38), 65535), (f(-1.0), 0), (f(-1e-9), 0),
            (f(np.nan), 0), (f(np.inf), 0), (f(-np.inf), 0), (f(1.0), 256), (f(100.25), 25664)]
