"""CPU: the float64 references of tests/fast_kernels_reference.py against the CPU oracle and the reference's own golden
outputs, so that the GPU tests that lean on them (test_cost_volume_mfma_gpu.py, test_cbca_separable_gpu.py) cannot be
fooled by a wrong restatement."""
import numpy as np
import pytest

import fast_kernels_reference as R
import tolerances as tol

U = 2.0 ** -24          # unit roundoff of float32


def pairwise32_bound(fl, fr, D):
    """A priori bound of NumPy's float32 pairwise sum of 64 products (8 running sums of 8, a 3-level tree, pf:87-91)
    against the exact dot product, per entry [D,H,W] of the left volume: every product is rounded once and then passes
    7 + 3 additions - (1 + u)^11 - 1 <= 12 u relative to sum |fl_c fr_c|."""
    a, b = np.abs(fl.astype(np.float64)), np.abs(fr.astype(np.float64))
    _, W, _ = fl.shape
    out = np.zeros((D,) + fl.shape[:2])
    for d in range(D):
        out[d, :, d:] = (a[:, d:] * b[:, :W - d]).sum(-1)
    return 12 * U * out


def check_scores(fl, fr, D, cv_l, cv_r, what):
    left, right, ml, mr = R.scores64(fl, fr, D)
    H, W, _ = fl.shape
    w, d = np.arange(W)[None, None, :], np.arange(D)[:, None, None]
    assert np.array_equal(ml, np.broadcast_to(w >= d, ml.shape)) and np.array_equal(mr, np.broadcast_to(w < W - d, mr.shape))
    bound = pairwise32_bound(fl, fr, D)
    el = np.abs(cv_l - left)
    assert (el[ml] <= bound[ml]).all(), "%s: left scores off by %g" % (what, (el - bound)[ml].max())
    for k in range(D):        # the right volume holds the same numbers, moved by d
        assert np.array_equal(right[k, :, :W - k], left[k, :, k:]), what
        assert np.array_equal(np.abs(cv_r[k, :, :W - k] - right[k, :, :W - k]) <= bound[k, :, k:],
                              np.ones((H, W - k), bool)), what
    return float(el[ml].max())


def test_scores64_against_the_reference_golden_volumes(golden_cases):
    for name, g in golden_cases:
        check_scores(g["fl"], g["fr"], g["cv_l"].shape[0], g["cv_l"], g["cv_r"], name)


def test_scores64_against_the_oracle_on_every_family():
    import oracle as o
    H, W, D = 2, 130, 64
    fams = R.feature_families(H, W, seed=1)
    assert set(fams) == {"gauss", "matched_0", "matched_3", "antiparallel", "near", "nonneg", "wide", "golden", "onehot",
                         "eighths"}
    e32 = {}
    for name, (fl, fr) in fams.items():
        for f in (fl, fr):
            assert f.dtype == np.float32 and f.shape == (H, W, 64) and np.abs(f).max() <= 1
            n = np.sqrt((f.astype(np.float64) ** 2).sum(-1))
            assert np.abs(n - 1).max() <= 64 * U / 2 + 4 * U, name       # unit to float32 rounding of 64 components
        cv_l, cv_r = o.compute_cost_volume(fl, fr, D)
        e32[name] = check_scores(fl, fr, D, cv_l, cv_r, name)
    # the matched families hold what the Gaussian one lacks: scores near -1 on the diagonal they were built for
    for name, d0 in (("matched_0", 0), ("matched_3", 3), ("nonneg", 0), ("wide", 0), ("near", 0)):
        left = R.scores64(*fams[name], D)[0]
        assert (left[d0, :, d0:] < -0.85).all(), name       # near: 1 / sqrt(1 + 64 * 0.05^2) = 0.93
    assert (R.scores64(*fams["antiparallel"], D)[0][0] > 0.999).all()
    assert np.abs(R.scores64(*fams["gauss"], D)[0]).max() < 0.7
    assert e32["onehot"] == 0 and e32["eighths"] == 0


def test_exact_families_have_exactly_representable_scores():
    for H, W, D in ((2, 130, 64), (2, 260, 256)):
        fams = R.feature_families(H, W, seed=2)
        left, _, ml, _ = R.scores64(*fams["onehot"], D)
        assert set(np.unique(left[ml])) == {-1.0, 0.0, 1.0}
        left, _, ml, _ = R.scores64(*fams["eighths"], D)
        k = left[ml] * 32
        assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 32 and np.unique(k).size > 20
        assert np.array_equal(left.astype(np.float32).astype(np.float64), left)


def test_region_mean64_against_the_reference_golden_aggregation(golden_cases):
    import oracle as o
    from helpers import hp_of
    for name, g in golden_cases:
        hp = hp_of(g)
        for side, img in (("l", "left"), ("r", "right")):
            arms, cv = g["arms_" + side], g["cv_" + side]
            assert np.array_equal(R.region_count(arms), g["region_num_" + side]), name
            mean = R.region_mean64(cv, arms)
            sp = float(np.spacing(np.float32(np.abs(cv).max())))
            assert np.abs(g["cbca1it_" + side] - mean).max() <= tol.CBCA_SPACINGS * sp, name
        l, r = o.cost_volume_aggregation(g["left"], g["right"], g["sgm_l"], g["sgm_r"], hp["cbca_intensity"],
                                         int(hp["cbca_distance"]), 1)
        for got, side in ((l, "l"), (r, "r")):
            sp = float(np.spacing(np.float32(np.abs(g["sgm_" + side]).max())))
            assert np.abs(got - R.region_mean64(g["sgm_" + side], g["arms_" + side])).max() <= tol.CBCA_SPACINGS * sp, name


def test_region_helpers_against_the_definition():
    import oracle as o
    H, W, L = 33, 70, 20
    arms, cnt = o.cross_arms(R.cbca_image(H, W, 1), R.CBCA_TAU, L)
    assert np.array_equal(cnt, R.region_count(arms))
    vol = R.cbca_volumes(2, H, W, 3)["mixed_scale"]
    mean = R.region_mean64(vol, arms)
    n_h, n_v = R.region_spans(arms)
    a = arms.astype(int)
    for h in range(0, H, 3):
        for w in range(0, W, 5):
            assert np.abs(mean[:, h, w] - R.region_mean_naive(vol, arms, h, w)).max() <= 2.0 ** -50
            rows = range(h - a[h, w, 0], h + a[h, w, 1] + 1)
            assert n_v[h, w] == len(rows) and n_h[h, w] == max(a[q, w, 2] + a[q, w, 3] + 1 for q in rows)
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.99999999) == 2.0 ** -24 and R.ulp32(0.0) == 2.0 ** -149
    assert R.ulp32(-3.0) == 2.0 ** -22 and R.ulp32(1e-45) == 2.0 ** -149


@pytest.mark.parametrize("H,W,D", R.CBCA_STREAM_SHAPES)
def test_stream_model_stays_inside_the_separable_tolerance(H, W, D):
    """The streaming kernel's algorithm, evaluated in NumPy on the inputs of test_cbca_separable_gpu.py (planes are
    independent: three per volume here), meets the tolerance that test asserts - and a float32 column prefix does not."""
    import oracle as o
    L = 14
    seed = R.cbca_case_seed(H, W, L)
    arms, cnt = o.cross_arms(R.cbca_image(H, W, seed), R.CBCA_TAU, L)
    assert cnt.max() > R.nontrivial_region_floor(H, W, L) and (cnt == 1).any()
    for name, vol in R.cbca_volumes(3 if D is None else min(D, 3), H, W, seed).items():
        mean = R.region_mean64(vol, arms)
        tolerance = R.separable_tolerance(mean, np.abs(vol).max())
        err = np.abs(R.stream_model64(vol, arms).astype(np.float64) - mean)
        assert (err <= tolerance).all(), "%s: %g of the tolerance" % (name, (err / tolerance).max())
        # (the mixed-scale sums are multiples of 2^-20 below 16, which float32 holds exactly: that volume is there for
        # cancellation, not for accumulation)
        if H >= 13 and name != "mixed_scale":
            hs = R._hsum64(vol.astype(np.float64), *R._arm_planes(arms)[2:])
            q32 = np.concatenate([np.zeros((vol.shape[0], 1, W), np.float32), np.cumsum(hs.astype(np.float32), axis=1,
                                                                                       dtype=np.float32)], axis=1)
            up, down = R._arm_planes(arms)[:2]
            hh = np.arange(H)[:, None]
            bad = (np.take_along_axis(q32, np.broadcast_to((hh + down + 1)[None], vol.shape), 1)
                   - np.take_along_axis(q32, np.broadcast_to((hh - up)[None], vol.shape), 1)).astype(np.float64) / cnt[None]
            assert (np.abs(bad - mean) > tolerance).any(), "%s: the tolerance would let a float32 column prefix pass" % name
