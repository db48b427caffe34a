"""GPU: the HIP path, called through the C ABI (libmccnn_hip.so via ctypes), against
  (1) the committed golden vectors produced by the reference itself, and
  (2) the CPU oracle on seeded inputs at sizes the oracle finishes in seconds.

Tolerances:
  bit-exact   cost volume (exact mode), arms/counts, CBCA (reference order), every SGM pass, WTA index, LR/interp,
              sub-pixel, median, bilateral
  <= 2e-6     cost volume on the matrix cores (split-f16 MFMA products instead of NumPy's pairwise order)
  <= 8 spacings of max|input| for one iteration, <= 2 per iteration over many - CBCA separable order (the correctly
              rounded mean against the reference's flat float32 running sum)
  <= 1e-5     features vs the float64-accumulating restatement (TensorFlow parity itself is unpinned)
"""
import numpy as np
import pytest
import torch

import tolerances as tol

from helpers import assert_bits, bits_equal, hp_of, module_setting

pytestmark = pytest.mark.gpu

DIRS = dict(right=(0, 1), left=(0, -1), up=(-1, 0), bottom=(1, 0))


@pytest.fixture(scope="module")
def pf():
    import _hipabi
    _hipabi.require_device()
    import process_functional
    return process_functional


@pytest.fixture(scope="module")
def sd():
    import stereo_device
    return stereo_device


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------
# (1) golden vectors
# ---------------------------------------------------------------------------------------------------------------
def test_golden_cost_volume_exact(pf, golden_cases):
    with module_setting(pf, "COST_VOLUME_MODE", "exact"):
        for name, g in golden_cases:
            l, r = pf.compute_cost_volume(g["fl"], g["fr"], g["cv_l"].shape[0])
            assert_bits(l, g["cv_l"], name + " cv_l")
            assert_bits(r, g["cv_r"], name + " cv_r")


def test_golden_cost_volume_mfma(pf, golden_cases):
    with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
        for name, g in golden_cases:
            l, r = pf.compute_cost_volume(g["fl"], g["fr"], g["cv_l"].shape[0])
            assert np.abs(l - g["cv_l"]).max() <= 2e-6, name
            assert np.abs(r - g["cv_r"]).max() <= 2e-6, name


def test_golden_cross_region(pf, sd, golden_cases):
    for name, g in golden_cases:
        hp = hp_of(g)
        for side in "lr":
            img = dev(g["left" if side == "l" else "right"][:, :, 0])
            sup = sd.cross_arms(img, hp["cbca_intensity"], int(hp["cbca_distance"]))
            assert np.array_equal(sd.support_arms(sup).cpu().numpy(), g["arms_" + side]), name
            assert np.array_equal(sd.support_count(sup).cpu().numpy(), g["region_num_" + side]), name
        if "region_l_crop" in g:
            reg, num = pf.compute_cross_region(g["left"], hp["cbca_intensity"], hp["cbca_distance"])
            assert reg.dtype == np.int32 and reg.shape == (g["left"].shape[0], g["left"].shape[1], 784, 2)
            assert np.array_equal(reg[:6, :8], g["region_l_crop"])
            assert np.array_equal(num, g["region_num_l"])


@pytest.mark.parametrize("order", ["reference", "reference_plane_major"])
def test_golden_cbca_reference_order_bit_exact(pf, golden_cases, order):
    """Both kernels that keep the reference's summation order: the pixel-major one behind the drop-in default and the
    plane-major one (round 2; still what distances > 14 use)."""
    with module_setting(pf, "CBCA_ORDER", order):
        for name, g in golden_cases:
            hp = hp_of(g)
            tau, dist = hp["cbca_intensity"], hp["cbca_distance"]
            cv_l = g["cv_l"].copy()
            l, r = pf.cost_volume_aggregation(g["left"], g["right"], cv_l, g["cv_r"], tau, dist, 1)
            assert_bits(l, g["cbca1it_l"], name)
            assert_bits(r, g["cbca1it_r"], name)
            assert_bits(cv_l, g["cv_l"], name + " (input untouched)")
            l, r = pf.cost_volume_aggregation(g["left"], g["right"], g["cv_l"], g["cv_r"], tau, dist, hp["it1"])
            assert_bits(l, g["cbca1_l"], name)
            assert_bits(r, g["cbca1_r"], name)
            l, r = pf.cost_volume_aggregation(g["left"], g["right"], g["sgm_l"], g["sgm_r"], tau, dist, hp["it2"])
            assert_bits(l, g["cbca2_l"], name)
            assert_bits(r, g["cbca2_r"], name)


def test_golden_cbca_separable_tolerance(pf, golden_cases):
    with module_setting(pf, "CBCA_ORDER", "separable"):
        _golden_cbca_separable_tolerance(pf, golden_cases)


def _golden_cbca_separable_tolerance(pf, golden_cases):
    for name, g in golden_cases:
        hp = hp_of(g)
        tau, dist = hp["cbca_intensity"], hp["cbca_distance"]
        # The streaming kernel returns the correctly rounded region mean; the reference's flat float32 running sum is
        # what carries the difference.  Bound in units of the float32 spacing at the largest input magnitude (the
        # summands' scale): <= 8 spacings for one iteration (measured <= 5), <= 2 per iteration over 16 (measured <= 18
        # in total at |costs| up to 160).
        l, r = pf.cost_volume_aggregation(g["left"], g["right"], g["cv_l"], g["cv_r"], tau, dist, 1)
        sp = float(np.spacing(np.float32(max(np.abs(g["cv_l"]).max(), np.abs(g["cv_r"]).max()))))
        assert np.abs(l - g["cbca1it_l"]).max() <= 8 * sp, name
        assert np.abs(r - g["cbca1it_r"]).max() <= 8 * sp, name
        l, r = pf.cost_volume_aggregation(g["left"], g["right"], g["sgm_l"], g["sgm_r"], tau, dist, hp["it2"])
        sp = float(np.spacing(np.float32(max(np.abs(g["sgm_l"]).max(), np.abs(g["sgm_r"]).max()))))
        assert np.abs(l - g["cbca2_l"]).max() <= 2 * hp["it2"] * sp, name
        assert np.abs(r - g["cbca2_r"]).max() <= 2 * hp["it2"] * sp, name


def test_golden_sgm_each_direction_bit_exact(pf, golden_cases):
    for name, g in golden_cases:
        hp = hp_of(g)
        for dname, r in DIRS.items():
            p1 = hp["sgm_P1"] if r[0] == 0 else hp["sgm_P1"] / hp["sgm_V"]
            for side, ch in (("l", "L"), ("r", "R")):
                v = g["cbca1_" + side].copy()
                out = pf.semi_global_matching(g["left"], g["right"], v, r, p1, hp["sgm_P2"], hp["sgm_Q1"],
                                              hp["sgm_Q2"], hp["sgm_D"], ch)
                assert out is v, "must mutate and return its argument (pf:544,568)"
                assert_bits(v, g["sgm_%s_%s" % (dname, side)], "%s sgm %s %s" % (name, dname, ch))


def test_golden_sgm_average_bit_exact(pf, golden_cases):
    for name, g in golden_cases:
        hp = hp_of(g)
        a, b = g["cbca1_l"].copy(), g["cbca1_r"].copy()
        l, r = pf.SGM_average(a, b, g["left"], g["right"], hp["sgm_P1"], hp["sgm_P2"], hp["sgm_Q1"], hp["sgm_Q2"],
                              hp["sgm_D"], hp["sgm_V"])
        assert_bits(l, g["sgm_l"], name + " sgm_l")
        assert_bits(r, g["sgm_r"], name + " sgm_r")
        assert_bits(a, g["sgm_l"], name + " argument mutated like the reference")


def test_golden_wta_to_bilateral_bit_exact(pf, golden_cases):
    for name, g in golden_cases:
        hp = hp_of(g)
        D = g["cv_l"].shape[0]
        dl, dr = pf.disparity_prediction(g["cbca2_l"], g["cbca2_r"])
        assert_bits(dl, g["wta_l"], name + " wta_l")
        assert_bits(dr, g["wta_r"], name + " wta_r")
        assert_bits(pf.interpolation(g["wta_l"], g["wta_r"], D), g["interp"], name + " interp")
        assert_bits(pf.subpixel_enhance(g["interp"], g["cbca2_l"]), g["subpixel"], name + " subpixel")
        assert_bits(pf.median_filter(g["subpixel"], 5, 5), g["median"], name + " median")
        assert_bits(pf.bilateral_filter(g["left"], g["median"], 5, 5, 0, hp["blur_sigma"], hp["blur_threshold"]),
                    g["bilateral"], name + " bilateral")


def test_golden_features(pf, golden_cases, net_layers):
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    for name, g in golden_cases:
        fl, fr = pf.compute_features(g["left"], g["right"], 11, 11, net)
        assert fl.shape == g["fl"].shape and fl.dtype == np.float32
        assert np.abs(fl - g["fl"]).max() <= 1e-5, name   # vs the float64-accumulating restatement
        assert np.abs(fr - g["fr"]).max() <= 1e-5, name
        # (f2) the row-banded evaluation straight against the same golden features (bands of 7 and 16 rows: several
        # bands with overlapped halos on the 24- and 40-row golden images)
        for rows in (7, 16):
            tl, tr = net.features_pair_hwc(dev(g["left"][:, :, 0]), dev(g["right"][:, :, 0]), tile_rows=rows)
            assert np.abs(tl.cpu().numpy() - g["fl"]).max() <= 1e-5, (name, rows)
            assert np.abs(tr.cpu().numpy() - g["fr"]).max() <= 1e-5, (name, rows)


@pytest.mark.parametrize("features", ["split_f16", "miopen"], ids=["hand_written_features_default", "library_features"])
def test_golden_whole_pair_reference_order(sd, golden_cases, net_layers, features):
    """StereoMatcher.match (the timed region) with the bit-exact stage variants, fed the golden features' images, with
    either feature path: the features differ from the oracle's float64-accumulating ones by 2.4e-7 .. 4.2e-7 (both
    paths), every stage behind them is bit-exact, so the final map is compared with a flip count and the two fractions
    of src/tolerances.py - the library path held to SURVEY App. D's 99.9 % within 1e-3 px, the hand-written path to the
    stated departure from it on one fixture.  Measured on the four golden pairs: 0 flips, every pixel
    within 1e-2 px; within 1e-3 px every pixel except on ref_40x48x16_s1, a pair with near-flat cost curves where the
    sub-pixel parabola turns 1e-7 into 1e-3 px: library features 3.5e-4 px at most, hand-written ones 1.2 % of the
    pixels at 1e-3 .. 4.3e-3 px."""
    import _hipabi as hip
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    for name, g in golden_cases:
        D = g["cv_l"].shape[0]
        m = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER, features=features)
        keep = {}
        out = m.match(dev(g["left"]), dev(g["right"]), D, keep=keep).cpu().numpy()
        flips = int((keep["wta"][0].cpu().numpy() != g["wta_l"]).sum())
        close = np.isclose(out, g["bilateral"], atol=1e-3, equal_nan=True).mean()
        close2 = np.isclose(out, g["bilateral"], atol=1e-2, equal_nan=True).mean()
        assert flips <= 2, "%s: %d WTA flips" % (name, flips)
        assert close >= tol.FEATURES_FINAL_MAP_FRAC_1E3[features], "%s: only %.4f of pixels within 1e-3 px" % (name, close)
        assert close2 >= tol.FEATURES_FINAL_MAP_FRAC_1E2, "%s: only %.4f of pixels within 1e-2 px" % (name, close2)


# ---------------------------------------------------------------------------------------------------------------
# (2) oracle on seeded inputs, mid sizes, ragged shapes
# ---------------------------------------------------------------------------------------------------------------
def _rand_vol(rng, D, H, W):
    return (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize("H,W,D", [(37, 83, 24), (70, 130, 64), (33, 300, 256), (20, 450, 400), (9, 21, 2)])
def test_oracle_sgm_passes_and_average(pf, H, W, D):
    import oracle as o
    import synthetic
    rng = np.random.default_rng(H * 1000 + W)
    L, R, _, _, _ = synthetic.make_pair(H, W, max(D, 4), seed=H + W)
    for r in DIRS.values():
        for ch in "LR":
            v0 = _rand_vol(rng, D, H, W)
            a, b = v0.copy(), v0.copy()
            o.semi_global_matching(L, R, a, r, 2.3, 55.9, 4, 8, 0.08, ch)
            pf.semi_global_matching(L, R, b, r, 2.3, 55.9, 4, 8, 0.08, ch)
            assert_bits(b, a, "sgm r=%s %s %dx%dx%d" % (r, ch, H, W, D))
    vl, vr = _rand_vol(rng, D, H, W), _rand_vol(rng, D, H, W)
    ol, orr = o.SGM_average(vl.copy(), vr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    gl, gr = pf.SGM_average(vl.copy(), vr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    assert_bits(gl, ol, "SGM_average L")
    assert_bits(gr, orr, "SGM_average R")


def test_oracle_sgm_penalty_classes_all_exercised(pf):
    """A high-contrast pair drives every (D1,D2) threshold combination, with non-power-of-two Q so P/Q rounds."""
    import oracle as o
    rng = np.random.default_rng(5)
    H, W, D = 24, 40, 16
    L = rng.choice([0.0, 0.05, 0.2, 1.0], size=(H, W, 1)).astype(np.float32)
    R = rng.choice([0.0, 0.07, 0.3, 1.0], size=(H, W, 1)).astype(np.float32)
    for r in DIRS.values():
        for ch in "LR":
            v0 = _rand_vol(rng, D, H, W)
            a, b = v0.copy(), v0.copy()
            o.semi_global_matching(L, R, a, r, 1.7, 31.3, 3, 7, 0.08, ch)
            pf.semi_global_matching(L, R, b, r, 1.7, 31.3, 3, 7, 0.08, ch)
            assert_bits(b, a, "sgm classes r=%s %s" % (r, ch))


@pytest.mark.parametrize("H,W,D", [(45, 100, 20), (64, 128, 33), (100, 70, 8)])
def test_oracle_cbca_and_cross(pf, sd, H, W, D):
    import oracle as o
    import synthetic
    rng = np.random.default_rng(W)
    L, R, _, _, _ = synthetic.make_pair(H, W, 16, seed=W)
    arms_o, cnt_o = o.cross_arms(L, 0.02, 14)
    sup = sd.cross_arms(dev(L[:, :, 0]), 0.02, 14)
    assert np.array_equal(sd.support_arms(sup).cpu().numpy(), arms_o)
    assert np.array_equal(sd.support_count(sup).cpu().numpy(), cnt_o)
    assert cnt_o.max() > 30, "test image must have non-trivial support regions"
    vl, vr = _rand_vol(rng, D, H, W), _rand_vol(rng, D, H, W)
    ol, orr = o.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 3)
    with module_setting(pf, "CBCA_ORDER", "reference"):
        gl, gr = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 3)
    assert_bits(gl, ol, "cbca reference order L")
    assert_bits(gr, orr, "cbca reference order R")
    with module_setting(pf, "CBCA_ORDER", "separable"):
        sl, sr = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 3)
    assert np.abs(sl - ol).max() <= 3e-6 and np.abs(sr - orr).max() <= 3e-6


def test_oracle_cbca_long_arms_other_distance(pf):
    """Flat image: every arm hits the distance limit; also a distance threshold other than the default 14."""
    import oracle as o
    rng = np.random.default_rng(1)
    H, W, D = 50, 90, 5
    L = np.zeros((H, W, 1), np.float32)
    R = np.zeros((H, W, 1), np.float32)
    R[:, ::7] = 1.0
    vl, vr = _rand_vol(rng, D, H, W), _rand_vol(rng, D, H, W)
    for dist in (14, 6, 20):
        ol, orr = o.cost_volume_aggregation(L, R, vl, vr, 0.02, dist, 2)
        with module_setting(pf, "CBCA_ORDER", "reference"):
            gl, gr = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, dist, 2)
        assert_bits(gl, ol, "flat image, distance %d" % dist)
        assert_bits(gr, orr, "striped image, distance %d" % dist)
        with module_setting(pf, "CBCA_ORDER", "separable"):
            sl, _ = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, dist, 2)
        assert np.abs(sl - ol).max() <= 2e-5   # up to (2*19+1)^2 terms per sum here


@pytest.mark.parametrize("H,W,D", [(21, 70, 40), (40, 200, 64), (12, 300, 256)])
def test_oracle_cost_volume(pf, H, W, D):
    import oracle as o
    rng = np.random.default_rng(D)
    fl = rng.standard_normal((H, W, 64)).astype(np.float32)
    fr = rng.standard_normal((H, W, 64)).astype(np.float32)
    fl /= np.linalg.norm(fl, axis=-1, keepdims=True)
    fr /= np.linalg.norm(fr, axis=-1, keepdims=True)
    ol, orr = o.compute_cost_volume(fl, fr, D)
    with module_setting(pf, "COST_VOLUME_MODE", "exact"):
        gl, gr = pf.compute_cost_volume(fl, fr, D)
    assert_bits(gl, ol, "cost volume L exact")
    assert_bits(gr, orr, "cost volume R exact")
    with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
        ml, mr = pf.compute_cost_volume(fl, fr, D)
    assert np.abs(ml - ol).max() <= 2e-6 and np.abs(mr - orr).max() <= 2e-6


def test_cost_volume_rejects_degenerate_disparity_range(pf):
    import _hipabi
    f = np.zeros((4, 10, 64), np.float32)
    with pytest.raises(_hipabi.MccnnHipError):
        pf.compute_cost_volume(f, f, 9)   # D > W-2: the reference's own border recurrence is degenerate there


@pytest.mark.parametrize("H,W,D", [(30, 50, 12), (64, 200, 70)])
def test_oracle_wta_ties_and_postprocessing(pf, H, W, D):
    import oracle as o
    rng = np.random.default_rng(H)
    # quantised costs -> many exact ties: the first minimum must win
    vl = (rng.integers(0, 6, size=(D, H, W)) * 0.25).astype(np.float32)
    vr = (rng.integers(0, 6, size=(D, H, W)) * 0.25).astype(np.float32)
    odl, odr = o.disparity_prediction(vl, vr)
    gdl, gdr = pf.disparity_prediction(vl, vr)
    assert_bits(gdl, odl, "wta ties L")
    assert_bits(gdr, odr, "wta ties R")
    # random maps exercise all three LR states and every interpolation branch
    dl = rng.integers(0, D, size=(H, W)).astype(np.float32)
    dr = rng.integers(0, D, size=(H, W)).astype(np.float32)
    dl[:, : W // 2] = 3.0
    dr[:, : W // 2] = 3.0
    st = o.lr_status(dl, dr, D)
    assert set(np.unique(st)) == {0, 1, 2}
    assert_bits(pf.interpolation(dl, dr, D), o.interpolation(dl, dr, D), "interpolation")
    di = o.interpolation(dl, dr, D)
    vol = rng.random((D, H, W), dtype=np.float32)
    osub = o.subpixel_enhance(di, vol)
    assert_bits(pf.subpixel_enhance(di, vol), osub, "subpixel")
    flat = np.zeros((D, H, W), np.float32)   # zero denominators -> nan/inf must propagate identically
    with np.errstate(all="ignore"):
        onan = o.subpixel_enhance(di, flat)
    gnan = pf.subpixel_enhance(di, flat)
    assert np.array_equal(np.isnan(onan), np.isnan(gnan))
    assert_bits(pf.median_filter(osub, 5, 5), o.median_filter(osub, 5, 5), "median 5x5")
    assert_bits(pf.median_filter(osub, 3, 7), o.median_filter(osub, 3, 7), "median 3x7")
    assert_bits(pf.median_filter(gnan, 5, 5), o.median_filter(onan, 5, 5), "median with nan")
    img = rng.standard_normal((H, W, 1)).astype(np.float32) * 2
    om = o.median_filter(osub, 5, 5)
    assert_bits(pf.bilateral_filter(img, om, 5, 5, 0, 6, 2), o.bilateral_filter(img, om, 5, 5, 0, 6, 2), "bilateral")
    assert_bits(pf.bilateral_filter(img, om, 3, 5, 0, 2.5, 0.7), o.bilateral_filter(img, om, 3, 5, 0, 2.5, 0.7),
                "bilateral 3x5")


@pytest.mark.parametrize("H,W", [(5, 1), (3, 64), (17, 65), (40, 129), (33, 257), (70, 700), (9, 1030)])
def test_oracle_interpolation_mask_kernels(pf, H, W):
    """The bit-mask interpolation (column carries + row masks) against the oracle's literal walks: widths on either
    side of the 64-pixel mask words and of the 256-thread row loop, rows and columns without any match, sparse and dense
    matches, all three states."""
    import oracle as o
    D = 40
    for dens, seed in ((0.5, 0), (0.03, 1), (0.97, 2)):
        rng = np.random.default_rng(seed + H * W)
        dl = rng.integers(0, D, size=(H, W)).astype(np.float32)
        # dr chosen so that a fraction `dens` of the pixels passes the left-right check
        dr = rng.integers(0, D, size=(H, W)).astype(np.float32)
        ok = rng.random((H, W)) < dens
        hh, ww = np.nonzero(ok)
        tgt = ww - dl[hh, ww].astype(np.int64)
        keep = tgt >= 0
        dr[hh[keep], tgt[keep]] = dl[hh[keep], ww[keep]]
        if H > 2:
            dl[H // 2, :] = D + 5.0          # a row of occlusions (disparity out of range)
        assert_bits(pf.interpolation(dl, dr, D), o.interpolation(dl, dr, D), "interpolation %dx%d %g" % (W, H, dens))


def test_cross_arms_pair_equals_two_calls(sd):
    """mccnn_cross_arms_pair (both views, one launch per kernel) writes the same three support planes as two
    mccnn_cross_arms calls."""
    g = torch.Generator(device="cuda").manual_seed(21)
    for H, W in ((37, 300), (64, 64), (5, 1)):
        a = torch.nn.functional.avg_pool2d(torch.rand((1, 1, H, W), device="cuda", generator=g), 3, 1, 1)[0, 0].contiguous()
        b = torch.nn.functional.avg_pool2d(torch.rand((1, 1, H, W), device="cuda", generator=g), 3, 1, 1)[0, 0].contiguous()
        sa, sb = sd.cross_arms(a, 0.02, 14), sd.cross_arms(b, 0.02, 14)
        pa, pb = sd.cross_arms_pair(a, b, 0.02, 14)
        v = -torch.rand((3, H, W), device="cuda", generator=g)
        for x, y in ((sa, pa), (sb, pb)):
            assert torch.equal(x, y)                       # arms + region sizes
            rx, _ = sd.cbca(v.clone(), torch.empty_like(v), x, 2, 14)   # the derived planes, through their consumer
            ry, _ = sd.cbca(v.clone(), torch.empty_like(v), y, 2, 14)
            assert torch.equal(rx, ry)


def test_layout_round_trip(sd):
    rng = np.random.default_rng(0)
    for (D, H, W) in [(5, 7, 9), (64, 33, 65), (130, 20, 70)]:
        v = rng.standard_normal((D, H, W)).astype(np.float32)
        hwd = sd.dhw_to_hwd(dev(v))
        assert hwd.shape == (H, W, (D + 3) // 4 * 4)
        assert np.array_equal(hwd.cpu().numpy()[:, :, :D], np.transpose(v, (1, 2, 0)))
        assert np.array_equal(sd.hwd_to_dhw(hwd, D).cpu().numpy(), v)


def test_torch_tensor_inputs_stay_on_device(pf):
    v = torch.rand((6, 12, 20), device="cuda") * -1
    dl, dr = pf.disparity_prediction(v, v)
    assert torch.is_tensor(dl) and dl.is_cuda and dl.shape == (12, 20)


# ---------------------------------------------------------------------------------------------------------------
# (3) full-size properties (no oracle at these sizes)
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_properties_cfg2(sd):
    """Middlebury-half sized volume (750x500, D=256): size-independent invariants of the kernels."""
    import _hipabi as hip
    H, W, D = 500, 750, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    v = -torch.rand((D, H, W), device="cuda", generator=g)
    # layout round trip is the identity
    hwd = sd.dhw_to_hwd(v)
    assert torch.equal(sd.hwd_to_dhw(hwd, D), v)
    # WTA == argmin (first minimum)
    assert torch.equal(sd.wta(v), torch.argmin(v, dim=0).float())
    # CBCA of a constant volume is that constant (averaging is a partition of unity) and is bounded by min/max
    img = (torch.rand((H, W), device="cuda", generator=g) * 4).round() / 4
    sup = sd.cross_arms(img, 0.02, 14)
    c = torch.full((4, H, W), -0.375, device="cuda")
    res, _ = sd.cbca(c, torch.empty_like(c), sup, 3, 14)
    assert torch.equal(res, torch.full_like(res, -0.375))
    res, _ = sd.cbca(v[:8].clone(), torch.empty((8, H, W), device="cuda"), sup, 2, 14)
    assert res.min() >= v[:8].min() - 1e-6 and res.max() <= v[:8].max() + 1e-6
    # SGM: adding a constant to the whole volume adds the same constant to the output of a pass (the recurrence adds
    # min(...) of the previous pixel and subtracts its min_k, which shift together) - checked on integer-valued
    # costs and dyadic penalties, where float32 arithmetic is exact
    vi = torch.randint(0, 64, (D, H, W), device="cuda", generator=g).float()
    scratch = sd.sgm_scratch(H, W, D, vi.device)
    outs = []
    for shift in (0.0, 32.0):
        h = sd.dhw_to_hwd(vi + shift)
        sd.sgm_pass_hwd(img, img, [h], [hip.MCCNN_SIDE_LEFT], D, (0, 1), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        sd.sgm_pass_hwd(img, img, [h], [hip.MCCNN_SIDE_LEFT], D, (1, 0), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        outs.append(sd.hwd_to_dhw(h, D))
    assert torch.equal(outs[1], outs[0] + 32.0)
    # first scan line of a pass is untouched
    h = sd.dhw_to_hwd(vi)
    sd.sgm_pass_hwd(img, img, [h], [hip.MCCNN_SIDE_RIGHT], D, (0, -1), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
    assert torch.equal(sd.hwd_to_dhw(h, D)[:, :, W - 1], vi[:, :, W - 1])


def test_full_size_cbca_streaming_vs_reference_order_cfg2(sd):
    """750x500: the streaming (float64 prefix) kernel against the bit-exact reference-order kernel, on a plane count
    that takes the multi-chunk launch (8 planes -> 7 row chunks) and on the single-chunk launch (256 planes, sampled).
    Tolerance: 1e-6 per iteration on O(1) costs (the reference's own float32 summation error)."""
    import _hipabi as hip
    H, W = 500, 750
    g = torch.Generator(device="cuda").manual_seed(3)
    img = torch.rand((H, W), device="cuda", generator=g)
    img = torch.nn.functional.avg_pool2d(img[None, None], 9, 1, 4)[0, 0].contiguous()   # smooth: long arms
    sup = sd.cross_arms(img, 0.02, 14)
    assert int(sd.support_count(sup).max()) > 200
    for D, sample in ((8, slice(None)), (256, slice(0, 256, 37))):
        v = -torch.rand((D, H, W), device="cuda", generator=g)
        fast, _ = sd.cbca(v.clone(), torch.empty_like(v), sup, 1, 14, hip.MCCNN_CBCA_SEPARABLE)
        vs = v[sample].contiguous()
        ref, _ = sd.cbca(vs.clone(), torch.empty_like(vs), sup, 1, 14, hip.MCCNN_CBCA_REFERENCE_ORDER)
        err = float((fast[sample] - ref).abs().max())
        assert err <= 1e-6, "D=%d: streaming vs reference order differ by %g" % (D, err)


@pytest.mark.parametrize("H,W,D,iters", [(500, 750, 256, 2), (375, 1242, 7, 3), (70, 300, 5, 1), (40, 33, 1, 2)])
def test_cbca_pair_launch_equals_two_single_launches(sd, H, W, D, iters):
    """mccnn_cbca_iter_pair (left + right volume dealt to one launch: whole rounds, chunked remainders, odd plane
    counts, one-strip images) is bit-identical to mccnn_cbca_iter on each volume; a reference-order request through
    the same entry point falls back to the two single launches."""
    import _hipabi as hip
    g = torch.Generator(device="cuda").manual_seed(11)
    imgs = [torch.nn.functional.avg_pool2d(torch.rand((1, 1, H, W), device="cuda", generator=g), 5, 1, 2)[0, 0]
            .contiguous() for _ in range(2)]
    sups = [sd.cross_arms(im, 0.02, 14) for im in imgs]
    vols = [-torch.rand((D, H, W), device="cuda", generator=g) for _ in range(2)]
    single = [sd.cbca(v.clone(), torch.empty_like(v), s_, iters, 14, hip.MCCNN_CBCA_SEPARABLE)[0]
              for v, s_ in zip(vols, sups)]
    (pl, _), (pr, _) = sd.cbca_pair(vols[0].clone(), torch.empty_like(vols[0]), sups[0], vols[1].clone(),
                                    torch.empty_like(vols[1]), sups[1], iters, 14, hip.MCCNN_CBCA_SEPARABLE)
    assert torch.equal(pl, single[0]) and torch.equal(pr, single[1])
    if D <= 8:
        ref = [sd.cbca(v.clone(), torch.empty_like(v), s_, 1, 14, hip.MCCNN_CBCA_REFERENCE_ORDER)[0]
               for v, s_ in zip(vols, sups)]
        (ql, _), (qr, _) = sd.cbca_pair(vols[0].clone(), torch.empty_like(vols[0]), sups[0], vols[1].clone(),
                                        torch.empty_like(vols[1]), sups[1], 1, 14, hip.MCCNN_CBCA_REFERENCE_ORDER)
        assert torch.equal(ql, ref[0]) and torch.equal(qr, ref[1])
    with pytest.raises(hip.MccnnHipError):      # outputs must not alias
        t = torch.empty_like(vols[0])
        sd.cbca_pair(vols[0], t, sups[0], vols[1], t, sups[1], 1, 14, hip.MCCNN_CBCA_SEPARABLE)


def test_full_size_sgm_first_pass_equals_unfused_cfg2(sd):
    """750x500x256: mccnn_sgm_first_pass (layout change fused into direction (0,1)) is bit-identical to
    mccnn_dhw_to_hwd followed by mccnn_sgm_pass, for both sides in one launch."""
    H, W, D = 500, 750, 256
    g = torch.Generator(device="cuda").manual_seed(5)
    il = torch.rand((H, W), device="cuda", generator=g)
    ir = torch.rand((H, W), device="cuda", generator=g)
    vl = -torch.rand((D, H, W), device="cuda", generator=g)
    vr = -torch.rand((D, H, W), device="cuda", generator=g)
    scratch = sd.sgm_scratch(H, W, D, vl.device)
    hp = dict(sgm_P1=2.3, sgm_P2=55.9, sgm_Q1=4.0, sgm_Q2=8.0, sgm_D=0.08, sgm_V=1.5)
    fused = [torch.empty((H, W, sd.hwd_pitch(D)), device="cuda") for _ in range(2)]
    sd.sgm_average_from_dhw(il, ir, [vl, vr], fused, [0, 1], D, scratch=scratch, **hp)
    plain = [sd.dhw_to_hwd(vl), sd.dhw_to_hwd(vr)]
    sd.sgm_average_hwd(il, ir, plain, [0, 1], D, scratch=scratch, **hp)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])


def test_full_size_properties_cfg4(sd):
    """1500x1000, D=400 (2.4 GB per volume: byte offsets beyond 2^31, D > 256 takes the two-group SGM kernel and the
    unfused layout change): the same invariants as at cfg2."""
    import _hipabi as hip
    H, W, D = 1000, 1500, 400
    g = torch.Generator(device="cuda").manual_seed(1)
    v = -torch.rand((D, H, W), device="cuda", generator=g)
    hwd = sd.dhw_to_hwd(v)
    back = sd.hwd_to_dhw(hwd, D)
    assert torch.equal(back, v)
    del back
    assert torch.equal(sd.wta(v), torch.argmin(v, dim=0).float())
    img = (torch.rand((H, W), device="cuda", generator=g) * 4).round() / 4
    sup = sd.cross_arms(img, 0.02, 14)
    tmp = torch.empty_like(v)
    c = torch.full_like(v, -0.375)
    res, _ = sd.cbca(c, tmp, sup, 1, 14)
    assert torch.equal(res, torch.full_like(res, -0.375))          # every plane, incl. those past 2^31 bytes
    del c, res
    res, _ = sd.cbca(v.clone(), tmp, sup, 1, 14)
    assert res.min() >= v.min() - 1e-6 and res.max() <= v.max() + 1e-6
    # last plane against the reference-order kernel run on that plane alone
    last = v[D - 1:].contiguous()
    ref, _ = sd.cbca(last.clone(), torch.empty_like(last), sup, 1, 14, hip.MCCNN_CBCA_REFERENCE_ORDER)
    assert float((res[D - 1:] - ref).abs().max()) <= 1e-6
    del res, tmp, ref
    # SGM shift invariance on exactly representable costs, horizontal then vertical, D = 400
    vi = torch.randint(0, 64, (D, H, W), device="cuda", generator=g).float()
    scratch = sd.sgm_scratch(H, W, D, vi.device)
    outs = []
    for shift in (0.0, 32.0):
        h = sd.dhw_to_hwd(vi + shift)
        sd.sgm_pass_hwd(img, img, [h], [hip.MCCNN_SIDE_LEFT], D, (0, 1), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        sd.sgm_pass_hwd(img, img, [h], [hip.MCCNN_SIDE_LEFT], D, (-1, 0), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        outs.append(sd.hwd_to_dhw(h, D))
        del h
    assert torch.equal(outs[1], outs[0] + 32.0)


def test_golden_whole_pair_fast_variants(sd, golden_cases, net_layers):
    """The shipped default (matrix-core cost volume, streaming CBCA) on the golden pairs against the reference's final
    map: the fast variants differ from the bit-exact ones by <= 2e-6 (cost volume) and <= 1e-6 per CBCA iteration, which
    can flip WTA ties; tolerance = the same flip budget as the bit-exact run with the GPU's own features."""
    import _hipabi as hip
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    for name, g in golden_cases:
        D = g["cv_l"].shape[0]
        m = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, cbca_order=hip.MCCNN_CBCA_SEPARABLE)
        keep = {}
        out = m.match(dev(g["left"]), dev(g["right"]), D, keep=keep).cpu().numpy()
        flips = int((keep["wta"][0].cpu().numpy() != g["wta_l"]).sum())
        close = np.isclose(out, g["bilateral"], atol=1e-3, equal_nan=True).mean()
        # measured: 0 flips on all four pairs; >= 98.85 % of the pixels within 1e-3 px (the sub-pixel parabola
        # amplifies 1e-6 cost differences where its denominator is small; largest difference 0.004 px)
        assert flips <= 2, "%s: %d WTA flips" % (name, flips)
        assert close >= tol.FAST_FRAC_WITHIN_1E3_PX, "%s: only %.4f of pixels within 1e-3 px" % (name, close)


def _random_shapes(n, seed):
    """Seeded ragged shapes: odd and even widths, single-strip and multi-strip images, heights below one row batch and
    above one row chunk, D down to 2 and not a multiple of 4; volumes small enough for the CPU checker."""
    rng = np.random.default_rng(seed)
    shapes = []
    while len(shapes) < n:
        H = int(rng.integers(3, 150))
        W = int(rng.integers(8, 420))
        D = int(rng.integers(2, min(W - 2, 260) + 1))
        if H * W * D <= 2_500_000:
            shapes.append((H, W, D))
    return shapes


@pytest.mark.parametrize("H,W,D", _random_shapes(10, seed=2024))
def test_oracle_random_shapes_fast_and_exact_kernels(pf, sd, H, W, D):
    """Every volume kernel against the CPU checker on seeded ragged shapes (the fixed cases above pick the shapes by
    hand; these are drawn): cost volume in both modes, both aggregation orders (one launch configuration per shape:
    strips, row chunks, odd-width instantiation), SGM_average through the fused first pass."""
    import oracle as o
    import synthetic
    rng = np.random.default_rng(H * 7919 + W * 31 + D)
    L, R, _, _, _ = synthetic.make_pair(H, W, max(D, 4), seed=H + W + D)
    # cost volume
    fl = rng.standard_normal((H, W, 64)).astype(np.float32)
    fr = rng.standard_normal((H, W, 64)).astype(np.float32)
    fl /= np.linalg.norm(fl, axis=-1, keepdims=True)
    fr /= np.linalg.norm(fr, axis=-1, keepdims=True)
    ol, orr = o.compute_cost_volume(fl, fr, D)
    with module_setting(pf, "COST_VOLUME_MODE", "exact"):
        gl, gr = pf.compute_cost_volume(fl, fr, D)
    assert_bits(gl, ol, "cost volume L exact %dx%dx%d" % (H, W, D))
    assert_bits(gr, orr, "cost volume R exact %dx%dx%d" % (H, W, D))
    with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
        ml, mr = pf.compute_cost_volume(fl, fr, D)
    assert np.abs(ml - ol).max() <= 2e-6 and np.abs(mr - orr).max() <= 2e-6, (H, W, D)
    # aggregation: reference order bit-exact, streaming kernel within the stated tolerance
    cl, cr = o.cost_volume_aggregation(L, R, ol, orr, 0.02, 14, 2)
    with module_setting(pf, "CBCA_ORDER", "reference"):
        rl, rr = pf.cost_volume_aggregation(L, R, ol, orr, 0.02, 14, 2)
    assert_bits(rl, cl, "cbca reference order L %dx%dx%d" % (H, W, D))
    assert_bits(rr, cr, "cbca reference order R %dx%dx%d" % (H, W, D))
    with module_setting(pf, "CBCA_ORDER", "separable"):
        sl, sr = pf.cost_volume_aggregation(L, R, ol, orr, 0.02, 14, 2)
    assert np.abs(sl - cl).max() <= 2e-6 and np.abs(sr - cr).max() <= 2e-6, (H, W, D)
    # SGM_average (fused first pass when D <= 256) is bit-exact
    if D >= 2:
        al, ar = o.SGM_average(cl.copy(), cr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
        bl, br = pf.SGM_average(cl.copy(), cr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
        assert_bits(bl, al, "SGM_average L %dx%dx%d" % (H, W, D))
        assert_bits(br, ar, "SGM_average R %dx%dx%d" % (H, W, D))


def test_abi_error_behaviour(sd):
    """Bad arguments come back as MCCNN_E_* with a message, never as a launch: null pointers, in-place aggregation,
    distances / disparity ranges the kernels are not built for."""
    import _hipabi as hip
    lib = hip.load()
    v = torch.zeros((4, 8, 16), device="cuda")
    img = torch.zeros((8, 16), device="cuda")
    sup = sd.cross_arms(img, 0.02, 14)
    s = hip.stream()
    assert lib.mccnn_cbca_iter(hip.ptr(v), hip.ptr(v), hip.ptr(sup), 4, 8, 16, 14, 0, s) == hip.MCCNN_E_INVALID
    assert b"in-place" in lib.mccnn_last_error_string()
    assert lib.mccnn_cbca_iter(None, hip.ptr(v), hip.ptr(sup), 4, 8, 16, 14, 0, s) == hip.MCCNN_E_INVALID
    out = torch.empty_like(v)
    assert lib.mccnn_cbca_iter(hip.ptr(v), hip.ptr(out), hip.ptr(sup), 4, 8, 16, 40, 0, s) == hip.MCCNN_E_UNSUPPORTED
    assert lib.mccnn_cbca_iter(hip.ptr(v), hip.ptr(out), hip.ptr(sup), 4, 8, 16, 14, 7, s) == hip.MCCNN_E_INVALID
    assert lib.mccnn_cross_arms(hip.ptr(img), 8, 16, 0.02, 33, hip.ptr(sup), s) == hip.MCCNN_E_UNSUPPORTED
    assert lib.mccnn_wta(hip.ptr(v), 0, 8, 16, hip.ptr(img), s) == hip.MCCNN_E_INVALID
    with pytest.raises(hip.MccnnHipError):
        hip.check(lib.mccnn_wta(None, 4, 8, 16, hip.ptr(img), s), "mccnn_wta")
    with pytest.raises(ValueError):
        sd.cbca(v, out, sup.clone(), 1, 14)      # a copy of the support tensor has lost its second plane


def test_graph_replay_equals_kernel_by_kernel(sd, net_layers):
    """StereoMatcher.match_graph (one hipGraph launch per pair, static buffers) against match() on three different
    pairs of one shape, fast and exact variants: bit-identical maps, and the replay really reuses its capture."""
    import _hipabi as hip
    import synthetic
    from model import NET
    H, W, D = 64, 96, 24
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    for cv, order, feat, hp, kern in (
            (hip.MCCNN_CV_MFMA, hip.MCCNN_CBCA_SEPARABLE, "miopen", None, "auto"),
            (hip.MCCNN_CV_MFMA, hip.MCCNN_CBCA_SEPARABLE, "split_f16", None, "auto"),   # bench.py --fast --separable-cbca
            (hip.MCCNN_CV_EXACT, hip.MCCNN_CBCA_REFERENCE_ORDER, "miopen", None, "auto"),
            # the drop-in default and --fast: the capture holds the side stream's two stages (arms + full programs
            # beside the cost volume, skip programs beside the first aggregation) with their event fork / join, and the
            # saturation-flag kernels of the hand-written features
            (hip.MCCNN_CV_EXACT, hip.MCCNN_CBCA_REFERENCE_ORDER, "split_f16", None, "auto"),
            (hip.MCCNN_CV_MFMA, hip.MCCNN_CBCA_REFERENCE_ORDER, "split_f16", None, "auto"),
            # fewer than three iterations in the second aggregation: no launch ever waits for the skip programs, the
            # join at the end of the aggregation is what brings the side stream back
            (hip.MCCNN_CV_EXACT, hip.MCCNN_CBCA_REFERENCE_ORDER, "split_f16", dict(cbca_num_iterations2=2), "auto"),
            (hip.MCCNN_CV_EXACT, hip.MCCNN_CBCA_REFERENCE_ORDER, "split_f16", dict(cbca_num_iterations2=1), "auto"),
            # no programs at all (cbca_hwd_kernel): the side stream carries the arms only
            (hip.MCCNN_CV_EXACT, hip.MCCNN_CBCA_REFERENCE_ORDER, "split_f16", None, "hwd")):
        m = sd.StereoMatcher(net, hp=hp, cv_mode=cv, cbca_order=order, features=feat, cbca_kernel=kern)
        if kern == "hwd":
            assert m.workspace(H, W, D)["progs"] is None
        for seed in (1, 2, 3):
            L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=seed)
            l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
            want = m.match(l, r, D).clone()
            got = m.match_graph(l, r, D)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), want.cpu().numpy(), equal_nan=True), (cv, order, feat, hp, kern, seed)
        assert len(m._graphs) == 1
