"""Plain NumPy restatements of the opt-in rules as include/mccnn.h defines them, and the inputs the two
paper-rules test files share.  No GPU, no fixtures.

None of the three rules is reference behaviour - they are what the MC-CNN paper does and the reference names and leaves
out, and the scalar promotion of the NumPy it was written for - so there is no reference output to compare with; the
checkers here are pinned against each other and against the oracle by test_paper_rules_cpu.py:

  interpolate_check, numpy1_subpixel_check, cbca_both_check   the literal loops test_extras_gpu.py has always used
  both_views_iter     one two-view aggregation, vectorised over voxels, each voxel in the kernel's order of additions
  interpolate_ex      mccnn_interpolate_ex for any status map and any float32 values (np.median decides NaN, -0.0)
  subpixel_numpy1     pf:396 under NumPy < 2's promotion, operation by operation as subpixel_kernel<true> states it
  match_paper         the whole timed region behind the cost volume with any set of extras
"""
import math
import warnings

import numpy as np

import oracle as o
import paper_sgm_reference as psr

F32, F64 = np.float32, np.float64

RAYS = [(1, 0), (1, 0.5), (1, 1), (0.5, 1), (0, 1), (-0.5, 1), (-1, 1), (-1, 0.5), (-1, 0), (-1, -0.5), (-1, -1),
        (-0.5, -1), (0, -1), (0.5, -1), (1, -1), (1, -0.5)]


# ---- the literal checkers of test_extras_gpu.py ---------------------------------------------------------------------
def interpolate_check(dl, st, directions, occ_left):
    H, W = dl.shape
    out = dl.copy()
    for h in range(H):
        for w in range(W):
            if st[h, w] == 1:
                nb = []
                if directions == 16:
                    for dx, dy in RAYS:
                        xx, yy = float(w), float(h)
                        while True:
                            xx += dx
                            yy += dy
                            xi, yi = int(math.floor(xx + 0.5)), int(math.floor(yy + 0.5))
                            if xi < 0 or xi >= W or yi < 0 or yi >= H:
                                break
                            if st[yi, xi] == 0:
                                nb.append(dl[yi, xi])
                                break
                else:
                    for rng_ in (range(w + 1, W), range(w - 1, -1, -1)):
                        for x in rng_:
                            if st[h, x] == 0:
                                nb.append(dl[h, x])
                                break
                    for rng_ in (range(h + 1, H), range(h - 1, -1, -1)):
                        for y in rng_:
                            if st[y, w] == 0:
                                nb.append(dl[y, w])
                                break
                if nb:
                    out[h, w] = np.median(np.array(nb, dtype=np.float32))
            elif st[h, w] == 2:
                for x in (range(w - 1, -1, -1) if occ_left else range(w + 1, W)):
                    if st[h, x] == 0:
                        out[h, w] = dl[h, x]
                        break
    return out


def numpy1_subpixel_check(d, vol):
    D, H, W = vol.shape
    want = d.copy()
    for h in range(H):
        for w in range(W):
            di = d[h, w]
            if int(di - 1) < 0 or int(di + 1) >= D:
                continue
            cm, cp, c = vol[int(di - 1), h, w], vol[int(di + 1), h, w], vol[int(di), h, w]
            num = np.float32(cp - cm)                               # float32 - float32 stays float32 under NumPy 1
            den = 2.0 * (np.float64(cp) - 2.0 * np.float64(c) + np.float64(cm))
            want[h, w] = np.float32(np.float64(di) - np.float64(num) / den)
    return want


def cbca_both_check(vol, arms_self, arms_other, side):
    """arms: uint8 [H,W,4] = up, down, left, right."""
    D, H, W = vol.shape
    out = np.empty_like(vol)
    for d in range(D):
        sh = -d if side == 0 else d
        for y in range(H):
            for x in range(W):
                def arms(qy):
                    a = arms_self[qy, x].astype(int)
                    xo = x + sh
                    if 0 <= xo < W:
                        a = np.minimum(a, arms_other[qy, xo].astype(int))
                    return a
                u, dn, _, _ = arms(y)
                s, n = np.float32(0), 0
                for qy in [y] + [y - k for k in range(1, u + 1)] + [y + k for k in range(1, dn + 1)]:
                    _, _, l, r = arms(qy)
                    for xx in [x] + [x - k for k in range(1, l + 1)] + [x + k for k in range(1, r + 1)]:
                        s = np.float32(s + vol[d, qy, xx])
                    n += l + r + 1
                out[d, y, x] = np.float32(s / np.float32(n))
    return out


# ---- two-view aggregation ---------------------------------------------------------------------------------------------
def clamp_of(L):
    """The R of the kernel instantiation that serves distance L: cbca_both_views_kernel<13,32> up to 14, <31,16> above."""
    return 13 if int(L) <= 14 else 31


def both_view_arms(arms_self, arms_other, side, D, R):
    """int32 [D,H,W,4]: the arms every voxel uses - own arms clamped to R, then min with the other view's at the partner
    column x - d (side 0, left) / x + d (side 1, right) where that column is inside the image."""
    own = np.minimum(np.asarray(arms_self).astype(np.int32), int(R))
    other = np.asarray(arms_other).astype(np.int32)
    H, W, _ = own.shape
    eff = np.empty((D, H, W, 4), dtype=np.int32)
    xs = np.arange(W)
    for d in range(D):
        xo = xs + (-d if side == 0 else d)
        ok = (xo >= 0) & (xo < W)
        eff[d] = own
        eff[d][:, ok] = np.minimum(own[:, ok], other[:, xo[ok]])
    return eff


def both_views_iter(vol, arms_self, arms_other, side, R):
    """One iteration of mccnn_cbca_iter_both on vol [D,H,W] float32.  Every voxel runs the same flat float32 sum the
    kernel runs - rows: self, up.., down..; within a row: self, left.., right..; the row's arms are those of (row, x)
    intersected at the SAME partner column - as a loop over the at most (2R+1)^2 steps, each applied to the voxels whose
    arms reach it; the count is accumulated row by row and divides once, in float32."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    D, H, W = vol.shape
    eff = both_view_arms(arms_self, arms_other, side, D, R)
    up, down = eff[..., 0], eff[..., 1]
    P = int(max(1, eff.max()))
    volp = np.zeros((D, H + 2 * P, W + 2 * P), dtype=np.float32)
    volp[:, P:P + H, P:P + W] = vol
    lrp = np.zeros((D, H + 2 * P, W, 2), dtype=np.int32)           # left / right arms, padded in y
    lrp[:, P:P + H] = eff[..., 2:]
    s = np.zeros((D, H, W), dtype=np.float32)
    n = np.zeros((D, H, W), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dq in [0] + [-k for k in range(1, int(up.max()) + 1)] + [k for k in range(1, int(down.max()) + 1)]:
            on = np.ones((D, H, W), dtype=bool) if dq == 0 else (up >= -dq if dq < 0 else down >= dq)
            if not on.any():
                continue
            left = np.where(on, lrp[:, P + dq:P + dq + H, :, 0], -1)
            right = np.where(on, lrp[:, P + dq:P + dq + H, :, 1], -1)
            rows = volp[:, P + dq:P + dq + H]
            np.add(s, rows[:, :, P:P + W], out=s, where=on)
            for z in range(1, int(left.max()) + 1):
                np.add(s, rows[:, :, P - z:P - z + W], out=s, where=left >= z)
            for z in range(1, int(right.max()) + 1):
                np.add(s, rows[:, :, P + z:P + z + W], out=s, where=right >= z)
            n += np.where(on, left + right + 1, 0)
        out = s / n.astype(np.float32)
    assert out.dtype == np.float32
    return out


def both_views(vol, arms_self, arms_other, side, R, iterations):
    for _ in range(int(iterations)):
        vol = both_views_iter(vol, arms_self, arms_other, side, R)
    return vol


# ---- interpolation ----------------------------------------------------------------------------------------------------
def interpolate_ex(dl, status, directions, occlusion_from_left, return_counts=False):
    """mccnn_interpolate_ex.  Status 1: np.median (float32 array: NaN wins, a median of -0.0 is +0.0) of the nearest
    status-0 values along 16 rays (positions rounded half up) or right, left, below, above; status 2: the nearest
    status-0 value to the left / right; the raw value where there is none and for every other status word.
    return_counts: also int32 [H,W], the number of neighbours a status-1 pixel found (-1 elsewhere)."""
    dl = np.ascontiguousarray(dl, dtype=np.float32)
    H, W = dl.shape
    st = np.asarray(status).tolist()                   # nested lists: the walks below index them a million times
    out = dl.copy()
    counts = np.full((H, W), -1, dtype=np.int32)
    assert directions in (4, 16)
    # positions in half pixels, so that the walk is integer arithmetic: a ray position k / 2 rounds half up to (k + 1) >> 1
    # (floor((k + 1) / 2), for negative k too); interpolate_check spells the same walk with floor(x + 0.5)
    rays = [(int(2 * dx), int(2 * dy)) for dx, dy in (RAYS if directions == 16 else [(1, 0), (-1, 0), (0, 1), (0, -1)])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # np.median announces every NaN it propagates
        for h in range(H):
            row = st[h]
            for w in range(W):
                s = row[w]
                if s == 1:
                    nb = []
                    for dx2, dy2 in rays:
                        x2, y2 = 2 * w, 2 * h
                        while True:
                            x2 += dx2
                            y2 += dy2
                            xi, yi = (x2 + 1) >> 1, (y2 + 1) >> 1
                            if xi < 0 or xi >= W or yi < 0 or yi >= H:
                                break
                            if st[yi][xi] == 0:
                                nb.append(dl[yi, xi])
                                break
                    counts[h, w] = len(nb)
                    if nb:
                        out[h, w] = np.median(np.array(nb, dtype=np.float32))
                elif s == 2:
                    for x in (range(w - 1, -1, -1) if occlusion_from_left else range(w + 1, W)):
                        if row[x] == 0:
                            out[h, w] = dl[h, x]
                            break
    return (out, counts) if return_counts else out


# ---- sub-pixel ------------------------------------------------------------------------------------------------------
def subpixel_numpy1(d, vol):
    """pf:396 as NumPy < 2 promotes it, in the steps of subpixel_kernel<true>: the three indices are int() of float32
    expressions; C+ - C- is a float32 difference; the denominator ((C+ - 2 C) + C-) * 2, the quotient and the subtraction
    are float64; one rounding to float32 at the end.  Unchanged where int(d - 1) < 0 or int(d + 1) >= D.  A non-finite
    disparity has no defined result (post_reference.subpixel_enhance)."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    D, H, W = vol.shape
    out = np.empty((H, W), dtype=np.float32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for h in range(H):
            for w in range(W):
                di = d[h, w]
                if not np.isfinite(di):
                    raise ValueError("subpixel_numpy1: a non-finite disparity has no defined result")
                im, ip, ic = int(F32(di - one)), int(F32(di + one)), int(di)
                if im < 0 or ip >= D:
                    out[h, w] = di
                    continue
                cm, cp, c = vol[im, h, w], vol[ip, h, w], vol[ic, h, w]
                num = F32(cp - cm)
                den = F64(cp) - F64(2.0) * F64(c)
                den = den + F64(cm)
                den = F64(2.0) * den
                out[h, w] = F32(F64(di) - F64(num) / den)
    return out


# ---- the whole pair -------------------------------------------------------------------------------------------------
EXTRAS_OFF = dict(both_view_support=False, interpolation_directions=4, occlusion_from_left=False, numpy1_promotion=False,
                  sgm_independent_directions=False)


def match_paper(left, right, cv_l, cv_r, ndisp, extras=None, hp=None):
    """paper_sgm_reference.match_from_cost_volumes with every extra: (final map, {stage: output}) under the names
    StereoMatcher.match(keep=...) uses.  Arms from oracle.cross_arms; WTA, lr_status, median and bilateral from the
    oracle; the opted-in stages from this module."""
    ex = dict(EXTRAS_OFF)
    ex.update(extras or {})
    a = dict(o.MATCH_DEFAULTS)
    a.update(hp or {})
    tau, dist = a["cbca_intensity"], int(a["cbca_distance"])
    sgm = [a[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]
    if ex["both_view_support"]:
        al, ar = o.cross_arms(left, tau, dist)[0], o.cross_arms(right, tau, dist)[0]
        R = clamp_of(dist)

        def aggregate(vl, vr, n):
            return both_views(vl, al, ar, 0, R, n), both_views(vr, ar, al, 1, R, n)
    else:
        def aggregate(vl, vr, n):
            return o.cost_volume_aggregation(left, right, vl, vr, tau, dist, n)
    c1 = aggregate(cv_l, cv_r, a["cbca_num_iterations1"])
    if ex["sgm_independent_directions"]:
        s = psr.SGM_average_independent(c1[0], c1[1], left, right, *sgm)
    else:
        s = o.SGM_average(c1[0].copy(), c1[1].copy(), left, right, *sgm)
    c2 = aggregate(s[0], s[1], a["cbca_num_iterations2"])
    dl, dr = o.disparity_prediction(c2[0], c2[1])
    st = o.lr_status(dl, dr, ndisp)
    di = interpolate_ex(dl, st, ex["interpolation_directions"], ex["occlusion_from_left"])
    ds = subpixel_numpy1(di, c2[0]) if ex["numpy1_promotion"] else o.subpixel_enhance(di, c2[0])
    dm = o.median_filter(ds, 5, 5)
    db = o.bilateral_filter(left, dm, 5, 5, 0, a["blur_sigma"], a["blur_threshold"])
    return db, dict(cbca1=c1, sgm=s, cbca2=c2, wta=(dl, dr), status=st, interp=di, subpixel=ds, median=dm, bilateral=db)


STAGES = ("cbca1", "sgm", "cbca2", "wta", "status", "interp", "subpixel", "median", "bilateral")


# ---- the inputs both test files share ------------------------------------------------------------------------------
def case_rng(*key):
    return np.random.default_rng([11] + [int(k) for k in key])


# two-view aggregation: (H, W, D, L).  Tiles are 64 columns x 32 rows up to L = 14 and 64 x 16 above: one tile less a
# row and a column, exactly one, one more, several in both directions; D = W + 2 has planes without any partner.
BOTH_SHAPES_SHORT = [(H, W, 7, L) for (H, W) in ((31, 63), (32, 64), (33, 65), (70, 130)) for L in (1, 2, 14)] \
    + [(33, 65, 67, 14)]
BOTH_SHAPES_LONG = [(H, W, 7, L) for (H, W) in ((17, 65), (40, 130)) for L in (15, 32)] + [(17, 65, 67, 32)]
IMAGE_PAIRS = ("constant/constant", "smooth/noise", "noise/smooth", "synthetic")
VOLUME_KINDS = ("random", "integer", "special")
CBCA_TAU = 0.02


def image_pair(kind, H, W, key):
    """Two float32 [H,W] views.  constant: every arm is L - 1 or the border; noise: (nearly) every arm is 0; smooth: a
    ramp of 0.004 per pixel along both axes, so an arm ends after 4 pixels (tau = 0.02)."""
    rng = case_rng(20, H, W, key)
    const = np.full((H, W), 0.25, dtype=np.float32)
    noise = rng.standard_normal((H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (0.004 * (xx + yy)).astype(np.float32)
    if kind == "constant/constant":
        return const, const.copy()
    if kind == "smooth/noise":
        return smooth, noise
    if kind == "noise/smooth":
        return noise, smooth
    import synthetic
    L, R, _, _, _ = synthetic.make_pair(H, W, 8, seed=6 + key)
    return np.ascontiguousarray(L[:, :, 0]), np.ascontiguousarray(R[:, :, 0])


def volume(kind, D, H, W, key):
    """random: (-1, 0] like a cost volume; integer: |c| <= 1023, every float32 sum over a region is exact; special: the
    random one with about 2 % NaN, +-inf and -0.0, and plane D // 2 all -0.0 (a sum of -0.0 that starts from +0 is +0)."""
    rng = case_rng(21, D, H, W, key)
    if kind == "integer":
        return rng.integers(-1023, 1024, size=(D, H, W)).astype(np.float32)
    v = (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    if kind == "special":
        hit = rng.random((D, H, W)) < 0.02
        v[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32), size=int(hit.sum()))
        v[D // 2] = F32(-0.0)
    return v


# interpolation
INTERP_SHAPES = [(1, 1), (1, 7), (7, 1), (6, 255), (6, 256), (6, 257), (3, 600), (37, 53)]
INTERP_MODES = [(4, False), (4, True), (16, False), (16, True)]
STATUS_KINDS = ("random", "all_mismatch", "all_match", "corner_match", "checkerboard", "border_block", "odd_words",
                "sparse")
MAP_KINDS = ("halves", "special")
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, -1.0], dtype=np.float32)


def status_map(kind, H, W, rng):
    st = rng.choice([0, 1, 2], size=(H, W), p=[0.3, 0.45, 0.25]).astype(np.int32)
    if kind == "all_mismatch":
        st[:] = 1
    elif kind == "all_match":
        st[:] = 0
    elif kind == "corner_match":
        st[:] = 1
        st[H - 1, W - 1] = 0
    elif kind == "checkerboard":
        yy, xx = np.mgrid[0:H, 0:W]
        st = ((yy + xx) & 1).astype(np.int32)
    elif kind == "border_block":
        st[:max(1, H // 2), :max(1, min(W, 9))] = 1        # mismatches with no match in some directions
    elif kind == "odd_words":
        hit = rng.random((H, W)) < 0.2
        st[hit] = rng.choice(np.array([3, -1, 7], dtype=np.int32), size=int(hit.sum()))
    elif kind == "sparse":                                 # few matches: a mismatch finds a few of its 16 rays answered
        st = rng.choice([0, 1, 2], size=(H, W), p=[0.04, 0.8, 0.16]).astype(np.int32)
    return st


def disparity_map(kind, H, W, rng):
    """halves: values k / 2, so that an even neighbour count averages two different values; special: 15 % NaN, +-inf,
    -0.0 and -1 wherever they fall - matched pixels included, which is what makes them neighbours."""
    m = (rng.integers(0, 40, size=(H, W)) / 2.0).astype(np.float32)
    if kind == "special":
        hit = rng.random((H, W)) < 0.15
        m[hit] = rng.choice(SPECIALS, size=int(hit.sum()))
    return m


def interpolation_cases(shape_index):
    """(status kind, map kind, dl, status) for one shape."""
    H, W = INTERP_SHAPES[shape_index]
    for si, sk in enumerate(STATUS_KINDS):
        for mi, mk in enumerate(MAP_KINDS):
            rng = case_rng(30, shape_index, si, mi)
            yield sk, mk, disparity_map(mk, H, W, rng), status_map(sk, H, W, rng)


# sub-pixel
SUBPIXEL_D = (2, 3, 4, 5, 12, 70, 257)
CURVE_KINDS = ("random", "flat", "nonfinite", "denormal", "huge")


def subpixel_case(D, kind):
    """(d [H,W], vol [D,H,W]).  Disparities: integers and, on 40 % of the pixels, x.5, D - 1.5, D - 1, >= D, -1, -0.0,
    -0.5, 1.25.  huge: costs near 1e38, where C+ - 2 C overflows in float32 and not in float64."""
    H, W = 5, 23
    rng = case_rng(40, D, CURVE_KINDS.index(kind))
    vol = rng.standard_normal((D, H, W)).astype(np.float32)
    if kind == "flat":
        vol[:] = F32(0.75)
    elif kind == "nonfinite":
        hit = rng.random((D, H, W)) < 0.3
        vol[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(hit.sum()))
    elif kind == "denormal":
        vol = (vol * F32(1e-40)).astype(np.float32)
    elif kind == "huge":
        with np.errstate(over="ignore"):
            vol = (vol * F32(1e38)).astype(np.float32)
    d = rng.integers(0, D, size=(H, W)).astype(np.float32)
    hit = rng.random((H, W)) < 0.4
    vals = np.array([0.5, 1.5, D - 1.5, D - 1, D - 0.5, D, D + 4, -1, -0.0, -0.5, 1.25], dtype=np.float32)
    d[hit] = rng.choice(vals, size=int(hit.sum()))
    return d, vol
