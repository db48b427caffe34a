#!/usr/bin/env python3
"""Generates tests/golden/route_*.npz by RUNNING THE REFERENCE ITSELF (dev container only), like gen_golden.py.

    python tests/golden/gen_route_golden.py [family ...]        # families: sgm cbca cv post (default: all)

The four ref_*.npz fixtures of gen_golden.py hold one scene class at the default hyper-parameters, D <= 16, W <= 48; on
the GPU they reach one SGM route, the distance <= 14 aggregation kernels and a cost volume of 16 planes.  The files
written here hold the smallest inputs at which every OTHER kernel route can still go wrong, one stage family per file,
with the reference's own outputs (process_functional.py through ref_shim.py; only numbers are written):

  route_sgm_d<D>.npz        one per class of sgm_route() (csrc/sgm_route.h), 3 x 6 pixels: the volume pair, the four
                            single-direction outputs per side, SGM_average per side
  route_sgm_pen130_<s>.npz  W > D at D = 130 on a pair that reaches all three penalty classes in every direction (asserted
                            below); one file per side
  route_cbca_d<D>.npz       a constant left image (every arm is the distance or the border) and a banded / quantised right
                            one; arms, region counts, aggregated volumes (and their WTA) at distances 1 .. 32
  route_cv_<H>x<W>x<D>.npz  unit features at C = 64 and the two cost volumes
  route_post_<H>x<W>x<D>.npz  a volume pair with ties; WTA, interpolation, sub-pixel, two medians, two bilaterals

They do not match ref_*.npz, so conftest.py's golden_cases sees what it saw before.  tests/test_reference_routes_cpu.py
(the oracle) and tests/test_reference_routes_gpu.py (every kernel route) read them.  All of them together take a few
minutes of CPU time; no file is larger than 1 MiB, and together they are no larger than the four ref_*.npz (asserted).
The budget decides what is thin: SGM files at D = 192, 256 and D >= 512 use dyadic penalties and costs (exact sums),
aggregation at D = 33 holds two (distance, iterations) cases and at D = 130 four on 4 rows, special values only at D = 3.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import arms_from_region  # noqa: E402
from route_fixtures import DIRS, POST_BILATERAL, POST_WINDOWS, SGM_CLASSES  # noqa: E402  (what the tests read)

MAX_FILE_BYTES = 1 << 20
SGM_HP = dict(sgm_P1=2.3, sgm_P2=55.9, sgm_Q1=4, sgm_Q2=8, sgm_D=0.08, sgm_V=1.5)
# multiples of 2**-1 throughout (P1 / V, P / Q included): with costs that are multiples of 2**-3 every sum is exact, so
# the outputs of the wide volumes (D >= 192, except 257) compress to a third and the files stay inside the size budget.
# Rounding - the order of additions - is pinned by the fixtures at the default penalties: D = 5, 130, 257 (two groups)
# and the penalty-class pair.
SGM_HP_DYADIC = dict(sgm_P1=4.0, sgm_P2=48.0, sgm_Q1=2, sgm_Q2=4, sgm_D=0.08, sgm_V=2.0)
CBCA_TAU = 0.02
_written = []


def save(name, out, hp):
    out = dict(out)
    for k, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            raise AssertionError("%s: %s is float64" % (name, k))
    assert name.startswith("route_")
    out["hp_names"] = np.array(sorted(hp), dtype="U32")
    out["hp_values"] = np.array([hp[k] for k in sorted(hp)], dtype=np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d KB)" % (path, size // 1024), flush=True)
    assert size <= MAX_FILE_BYTES, "%s is larger than 1 MiB" % name
    _written.append(size)


# ---- SGM ----------------------------------------------------------------------------------------------------------------
def sgm_outputs(pf, L, R, vols, hp):
    out = {}
    for side, ch in (("l", "L"), ("r", "R")):
        for name, r in DIRS.items():
            p1 = hp["sgm_P1"] if r[0] == 0 else hp["sgm_P1"] / hp["sgm_V"]
            out["sgm_%s_%s" % (name, side)] = pf.semi_global_matching(
                L, R, vols[side].copy(), r, p1, hp["sgm_P2"], hp["sgm_Q1"], hp["sgm_Q2"], hp["sgm_D"], ch)
    al, ar = pf.SGM_average(vols["l"].copy(), vols["r"].copy(), L, R, hp["sgm_P1"], hp["sgm_P2"], hp["sgm_Q1"],
                            hp["sgm_Q2"], hp["sgm_D"], hp["sgm_V"])
    out["avg_l"], out["avg_r"] = al, ar
    return out


def penalty_classes(L, R, D, r, thr, choice):
    """{1, 2, 3}: which of pf:535-537's conditions occur on the pixels the pass of direction r visits."""
    own, other = (L, R) if choice == "L" else (R, L)
    own, other = own[:, :, 0], other[:, :, 0]
    H, W = own.shape
    rh, rw = r
    seen = set()
    for h in range(max(rh, 0), H + min(rh, 0)):
        for w in range(max(rw, 0), W + min(rw, 0)):
            d1 = abs(own[h, w] - own[h - rh, w - rw])
            for d in range(D):
                a, b = (w - d, w - rw - d) if choice == "L" else (w + d, w - rw + d)
                d2 = np.float32(0) if min(a, b) < 0 or max(a, b) >= W else abs(other[h, a] - other[h - rh, b])
                seen.add(1 if d1 < thr and d2 < thr else 2 if d1 >= thr and d2 >= thr else 3)
    return seen


def gen_sgm(pf):
    for D in SGM_CLASSES:
        rng = np.random.default_rng(1000 + D)
        H, W = 3, 6
        rounding = D < 192 or D == 257          # default penalties: sums round (one multi-group class among them)
        hp = SGM_HP if rounding else SGM_HP_DYADIC
        # grey levels 0.04 apart: a step of two levels lands on sgm_D = 0.08
        L = (rng.integers(0, 4, (H, W, 1)) * np.float32(0.04)).astype(np.float32)
        R = (rng.integers(0, 4, (H, W, 1)) * np.float32(0.04)).astype(np.float32)
        if rounding:    # small integers * 2**-10 below 32: every candidate of the minimum (pf:555-558) wins somewhere
            vols = {s: (rng.integers(0, 1 << 15, (D, H, W)) * np.float32(2.0 ** -10)).astype(np.float32) for s in "lr"}
        elif D < 512:
            vols = {s: (rng.integers(0, 1 << 9, (D, H, W)) * np.float32(2.0 ** -3)).astype(np.float32) for s in "lr"}
        else:           # halves below 64: the widest files compress best, and the minimum over the line has many ties
            vols = {s: (rng.integers(0, 1 << 7, (D, H, W)) * np.float32(0.5)).astype(np.float32) for s in "lr"}
        out = dict(left=L, right=R, vol_l=vols["l"], vol_r=vols["r"])
        with ref_shim.quiet():
            out.update(sgm_outputs(pf, L, R, vols, hp))
        save("route_sgm_d%d" % D, out, hp)

    # W > D at D = 130: the D2 term (pf:517-520 / 530-533) is live for most (w, d)
    rng = np.random.default_rng(130)
    H, W, D = 3, 131, 130
    L = rng.choice([0.0, 0.05, 0.2, 1.0], size=(H, W, 1)).astype(np.float32)
    R = rng.choice([0.0, 0.07, 0.3, 1.0], size=(H, W, 1)).astype(np.float32)
    for r in DIRS.values():
        for ch in "LR":
            assert penalty_classes(L, R, D, r, np.float32(SGM_HP["sgm_D"]), ch) == {1, 2, 3}, (r, ch)
    vols = {s: (rng.integers(0, 1 << 15, (D, H, W)) * np.float32(2.0 ** -10)).astype(np.float32) for s in "lr"}
    with ref_shim.quiet():
        res = sgm_outputs(pf, L, R, vols, SGM_HP)
    for s in "lr":
        out = dict(left=L, right=R)
        out["vol_" + s] = vols[s]
        out.update({k: v for k, v in res.items() if k.endswith("_" + s)})
        save("route_sgm_pen130_" + s, out, SGM_HP)


# ---- aggregation --------------------------------------------------------------------------------------------------------
def cbca_images(H, W):
    """Left: constant.  Right: vertical bands of grey levels 0.02 apart (a step of one level lands on the arm test's
    threshold, pf:588), a block of three-level noise, and isolated pixels whose region is the pixel itself."""
    rng = np.random.default_rng(H * 1000 + W)
    L = np.full((H, W, 1), np.float32(0.5), dtype=np.float32)
    level = np.zeros((H, W), dtype=np.int64)
    edges = [0, 3, 4, 12, 29, 30, 47, W]
    for k in range(len(edges) - 1):
        level[:, edges[k]:edges[k + 1]] = (0, 1, 3, 4, 2, 3, 5)[k]
    level[H // 2:, 47:] = rng.integers(0, 3, (H - H // 2, W - 47))
    for (h, w) in ((1, 7), (2, 20), (H - 2, 35), (0, 0), (H - 1, 14), (3, 46)):
        level[h % H, w] = 9
    R = (level * np.float32(CBCA_TAU)).astype(np.float32)[:, :, None]
    return L, R


def plant(vol, rng, values, n):
    idx = rng.choice(vol.size, n, replace=False)
    vol.reshape(-1)[idx] = np.asarray(values, np.float32)[rng.integers(0, len(values), n)]


def gen_cbca(pf):
    # (D, H, W, ((distance, iterations), ...), distance of the case with special values or None)
    plans = ((3, 20, 70, tuple((L, it) for L in (1, 14, 15, 28, 32) for it in (1, 3)), 14),
             (33, 20, 70, ((14, 3), (28, 3)), None),
             (130, 4, 70, ((14, 3), (15, 1), (28, 3), (32, 3)), None))
    for D, H, W, cases, special in plans:
        rng = np.random.default_rng(D)
        L, R = cbca_images(H, W)
        vl = (rng.integers(-1024, 1, (D, H, W)) * np.float32(2.0 ** -10)).astype(np.float32)   # [-1, 0] like real costs
        vr = (rng.integers(-1024, 1, (D, H, W)) * np.float32(2.0 ** -10)).astype(np.float32)
        out = dict(left=L, right=R, vol_l=vl, vol_r=vr, cases=np.array(cases, dtype=np.int32))
        equal = False
        with ref_shim.quiet():
            for dist in sorted(set(c[0] for c in cases)):
                for s, img in (("l", L), ("r", R)):
                    reg, num = pf.compute_cross_region(img, CBCA_TAU, dist)
                    arms = arms_from_region(reg, num)
                    out["arms_%s_L%d" % (s, dist)], out["num_%s_L%d" % (s, dist)] = arms, num
                    if s == "l":          # constant image: every arm is the distance or the border
                        hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
                        want = [np.minimum(x, dist - 1) + 0 * y for x, y in ((hh, ww), (H - 1 - hh, ww), (ww, hh),
                                                                             (W - 1 - ww, hh))]
                        assert np.array_equal(arms, np.stack(want, -1).astype(np.uint8))
                # an arm of the right image that ends on |difference| == threshold exactly (the `>=` of pf:588)
                a, g = out["arms_r_L%d" % dist], R[:, :, 0]
                for h in range(H):
                    for w in range(W - 1):
                        rt = int(a[h, w, 3])
                        if rt < dist - 1 and w + rt + 1 < W:
                            equal |= abs(g[h, w] - g[h, w + rt + 1]) == np.float32(CBCA_TAU)
            for dist, its in cases:
                al, ar = pf.cost_volume_aggregation(L, R, vl, vr, CBCA_TAU, dist, its)
                key = "L%d_it%d" % (dist, its)
                out["agg_l_" + key], out["agg_r_" + key] = al, ar
                out["wta_l_" + key], out["wta_r_" + key] = pf.disparity_prediction(al, ar)
            if special is not None:
                sl, sr = vl.copy(), vr.copy()
                plant(sl, rng, [np.inf, -np.inf, -0.0], 12)
                plant(sr, rng, [np.inf, -np.inf, -0.0], 12)
                sr[:, 1, 7] = -0.0                    # a unit-region pixel of the right image: -0.0 -> +0.0 (pf:157-161)
                assert out["num_r_L%d" % special][1, 7] == 1
                out["special_vol_l"], out["special_vol_r"] = sl, sr
                out["special_distance"] = np.int32(special)
                for its in (1, 3):
                    al, ar = pf.cost_volume_aggregation(L, R, sl, sr, CBCA_TAU, special, its)
                    out["special_agg_l_it%d" % its], out["special_agg_r_it%d" % its] = al, ar
        assert equal, "no arm ends on an intensity difference equal to the threshold"
        assert (out["num_r_L%d" % cases[0][0]] == 1).sum() >= 4, "the right image needs unit regions"
        save("route_cbca_d%d" % D, out, dict(cbca_intensity=CBCA_TAU))


# ---- cost volume --------------------------------------------------------------------------------------------------------
def unit_features(rng, H, W, C=64):
    f = rng.standard_normal((H, W, C)).astype(np.float32)
    return (f / np.sqrt((f * f).sum(-1, keepdims=True))).astype(np.float32)


def gen_cv(pf):
    for H, W, D, special in ((3, 42, 40, False), (2, 132, 130, False), (2, 300, 256, False), (3, 42, 40, True)):
        rng = np.random.default_rng(H * W + D + int(special))
        fl, fr = unit_features(rng, H, W), unit_features(rng, H, W)
        if special:
            fl[1, 20, 5], fl[2, 3, 0] = np.nan, np.inf
            fr[0, 30, 63], fr[2, 39, 1] = np.inf, np.nan
        with ref_shim.quiet(), np.errstate(all="ignore"):
            cl, cr = pf.compute_cost_volume(fl, fr, D)
        if special:
            assert np.isnan(cl).any() and np.isinf(cl).any()
        name = "route_cv_%dx%dx%d%s" % (H, W, D, "_special" if special else "")
        if cl.nbytes + cr.nbytes > MAX_FILE_BYTES * 0.8:      # the widest volume: one file per side
            save(name + "_l", dict(fl=fl, fr=fr, cv_l=cl), {})
            save(name + "_r", dict(fl=fl, fr=fr, cv_r=cr), {})
        else:
            save(name, dict(fl=fl, fr=fr, cv_l=cl, cv_r=cr), {})


# ---- WTA .. bilateral -------------------------------------------------------------------------------------------------
def post_volumes(rng, H, W, D):
    """Costs in halves (ties, pf:250's strict `<` keeps the first): noise in [2, 6], and on three quarters of the pixels
    a planted minimum at a block-wise constant disparity, the same on both sides - matches, mismatches and occlusions."""
    vols = []
    dmap = rng.integers(0, D, (2, 4))[np.arange(H)[:, None] * 2 // H, np.arange(W)[None, :] * 4 // W]
    for _ in range(2):
        v = (rng.integers(4, 13, (D, H, W)) * np.float32(0.5)).astype(np.float32)
        hit = rng.random((H, W)) < 0.75
        hh, ww = np.nonzero(hit)
        v[dmap[hh, ww], hh, ww] = rng.integers(0, 4, hh.size) * np.float32(0.5)
        vols.append(v)
    return vols


def gen_post(pf):
    for H, W, D in ((6, 255, 8), (6, 256, 8), (6, 257, 8), (9, 40, 256)):
        rng = np.random.default_rng(H * W + D)
        vl, vr = post_volumes(rng, H, W, D)
        img = (rng.integers(0, 6, (H, W, 1)) * np.float32(0.7)).astype(np.float32)
        out = dict(vol_l=vl, vol_r=vr, left=img)
        with ref_shim.quiet(), np.errstate(all="ignore"):
            dl, dr = pf.disparity_prediction(vl, vr)
            out["wta_l"], out["wta_r"] = dl, dr
            di = pf.interpolation(dl, dr, D)
            out["interp"] = di
            ds = pf.subpixel_enhance(di, vl)
            out["subpixel"] = ds
            for fh, fw in POST_WINDOWS:
                out["median_%dx%d" % (fh, fw)] = pf.median_filter(ds, fh, fw)
            dm = out["median_5x5"]
            for sigma, thr in POST_BILATERAL:
                out["bilateral_s%g_t%g" % (sigma, thr)] = pf.bilateral_filter(img, dm, 5, 5, 0, sigma, thr)
        assert (dl != di).any(), "no pixel was interpolated"
        assert np.isfinite(ds).mean() > 0.9
        save("route_post_%dx%dx%d" % (H, W, D), out, {})


FAMILIES = dict(sgm=gen_sgm, cbca=gen_cbca, cv=gen_cv, post=gen_post)


def main(argv):
    assert ref_shim.available(), "the reference is only present in the dev container"
    pf, _util = ref_shim.load_reference()
    for fam in (argv or sorted(FAMILIES)):
        t0 = time.time()
        FAMILIES[fam](pf)
        print("%s: %.1f s" % (fam, time.time() - t0), flush=True)
    print("%d files written, %d KB together" % (len(_written), sum(_written) // 1024))
    # the budget of all route files on disk: no more than the four whole-pair fixtures together
    import glob
    total = sum(os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "route_*.npz")))
    budget = sum(os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "ref_*.npz")))
    print("route_*.npz: %d bytes of %d" % (total, budget))
    assert total <= budget, "route_*.npz together are larger than ref_*.npz together"


if __name__ == "__main__":
    main(sys.argv[1:])
