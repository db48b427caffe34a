"""GPU: parity at the sizes of BASELINE.json's configs.

cfg1 (256x256, D=64) is small enough for the CPU checker to follow a WHOLE pair stage by stage (each stage of the GPU
run is fed, on the CPU, the GPU's own output of the stage before - identical inputs, so the bit-exact variants must be
bit-identical and the fast variants stay within their stated per-stage tolerance).  The measured differences are written
to gpurun_out/parity_r03.json (copied to profiles/ by hand) so that the numbers behind the bounds are on record.
cfg3 (1242x375, D=192) gets the size-independent properties and an oracle window at its full width.
"""
import json
import os

import numpy as np
import pytest
import torch

import tolerances as tol

from conftest import ROOT
from helpers import assert_bits, module_setting, stagewise

pytestmark = pytest.mark.gpu

RECORD = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dump():
    out_dir = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "parity_r03.json"), "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


def test_cfg1_whole_pair_stage_by_stage(net_layers):
    """BASELINE cfg1, one synthetic pair through the whole timed region, both variants."""
    import _hipabi as hip
    import oracle as o
    import stereo_device as sd
    import synthetic
    from model import NET
    H, W, D = 256, 256, 64
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=11)
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)

    # bit-exact variants: every stage after the features bit-identical given the GPU's own previous output
    m = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
    keep = {}
    exact_map = m.match(dev(L), dev(R), D, keep=keep).cpu().numpy()
    assert m.features == "split_f16"          # the default: the hand-written conv stack (deterministic, no library)
    fl = net.features_pair_hwc_split(dev(L[:, :, 0]), dev(R[:, :, 0]))
    ocv = o.compute_cost_volume(fl[0].cpu().numpy(), fl[1].cpu().numpy(), D)
    assert_bits(keep["cv"][0].cpu().numpy(), ocv[0], "cfg1 cost volume L")
    assert_bits(keep["cv"][1].cpu().numpy(), ocv[1], "cfg1 cost volume R")
    d = stagewise(keep, L, R, D, o)
    RECORD["cfg1_exact_stagewise_max_abs"] = d
    bad = {k: v for k, v in d.items() if v != 0}
    assert not bad, "bit-exact variants differ from the CPU checker: %s" % bad
    exact_wta = keep["wta"][0].cpu().numpy()
    ofl = o.net_features(L, net_layers)
    RECORD["cfg1_features_max_abs_vs_float64_restatement"] = float(np.abs(fl[0].cpu().numpy() - ofl).max())
    assert RECORD["cfg1_features_max_abs_vs_float64_restatement"] <= 1e-5

    # fast variants: per-stage tolerance against the CPU checker on identical inputs, then against the exact run
    m = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, cbca_order=hip.MCCNN_CBCA_SEPARABLE)
    keep = {}
    fast_map = m.match(dev(L), dev(R), D, keep=keep).cpu().numpy()
    cv_err = max(float(np.abs(keep["cv"][0].cpu().numpy() - ocv[0]).max()),
                 float(np.abs(keep["cv"][1].cpu().numpy() - ocv[1]).max()))
    d = stagewise(keep, L, R, D, o)
    d["cost_volume_mfma"] = cv_err
    flips = int((keep["wta"][0].cpu().numpy() != exact_wta).sum())
    close = float(np.isclose(fast_map, exact_map, atol=1e-3, equal_nan=True).mean())
    RECORD["cfg1_fast_stagewise_max_abs"] = d
    RECORD["cfg1_fast_vs_exact"] = {"wta_flips": flips, "pixels": int(fast_map.size),
                                    "fraction_within_1e-3_px": close,
                                    "max_abs_px": float(np.nanmax(np.abs(fast_map - exact_map)))}
    # the same fast variants with the conv features from the split-operand matrix-core kernels (what --fast and bench.py
    # run): features against the float64 restatement, final map against the bit-exact run
    sfl = net.features_pair_hwc_split(dev(L[:, :, 0]), dev(R[:, :, 0]))
    RECORD["cfg1_split_features_max_abs_vs_float64_restatement"] = float(np.abs(sfl[0].cpu().numpy() - ofl).max())
    m = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, cbca_order=hip.MCCNN_CBCA_SEPARABLE, features="split_f16")
    keep_s = {}
    split_map = m.match(dev(L), dev(R), D, keep=keep_s).cpu().numpy()
    flips_s = int((keep_s["wta"][0].cpu().numpy() != exact_wta).sum())
    close_s = float(np.isclose(split_map, exact_map, atol=1e-3, equal_nan=True).mean())
    RECORD["cfg1_fast_with_split_features_vs_exact"] = {
        "wta_flips": flips_s, "pixels": int(split_map.size), "fraction_within_1e-3_px": close_s,
        "max_abs_px": float(np.nanmax(np.abs(split_map - exact_map)))}
    _dump()
    assert RECORD["cfg1_split_features_max_abs_vs_float64_restatement"] <= 1e-5
    assert flips_s <= tol.FAST_WTA_FLIP_FRACTION * split_map.size, "split features: %d WTA flips of %d" % (flips_s, split_map.size)
    assert close_s >= tol.FAST_FRAC_WITHIN_1E3_PX, "split features: only %.4f of the pixels within 1e-3 px of the bit-exact run" % close_s
    assert cv_err <= 2e-6
    assert d["cbca_x2"] <= 2 * 8 * float(np.spacing(np.float32(1.0)))          # <= 8 spacings of max|input| per iteration
    # 16 iterations on post-SGM costs (|v| up to ~200), regions up to 729 pixels: measured 60 spacings of max|input|
    # (9.2e-4 absolute) - the reference's flat float32 running sum is what deviates from the correctly rounded mean
    assert d["cbca_x16_spacings_of_max_input"] <= 8.0 * 16
    for k in ("sgm", "interpolation", "subpixel", "median", "bilateral"):       # these stages have no fast variant
        assert d[k] == 0.0, (k, d[k])
    assert d["wta_mismatches"] == 0
    assert flips <= tol.FAST_WTA_FLIP_FRACTION * fast_map.size, "fast variants flip %d WTA decisions of %d" % (flips, fast_map.size)
    assert close >= tol.FAST_FRAC_WITHIN_1E3_PX, "only %.4f of the pixels within 1e-3 px of the bit-exact run" % close


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg4"])
def test_benchmarked_path_against_bit_exact_variant_full_size(net_layers, cfg):
    """What bench.py times - fast variants + split-operand features, replayed as one hipGraph - at BASELINE's full
    sizes: (1) the replay is bit-identical to the same matcher launched kernel by kernel; (2) against the bit-exact
    variant (oracle-pinned stage by stage at cfg1 and on ragged shapes, hence the full-size proxy for the reference):
    index-exact WTA up to a handful of near-ties, final map within the fast variant's stated tolerance; (3) the
    bit-exact variant on pixel-major volumes equals its plane-major twin bit for bit."""
    import _hipabi as hip
    import stereo_device as sd
    import synthetic
    from bench import CONFIGS
    from model import NET
    H, W, D = CONFIGS[cfg]
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=100)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    fast = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_MFMA, cbca_order=hip.MCCNN_CBCA_SEPARABLE, features="split_f16")
    replay = fast.match_graph(l, r, D).clone()
    kf = {}
    eager = fast.match(l, r, D, keep=kf)
    assert torch.equal(replay.view(torch.int32), eager.view(torch.int32)), "graph replay differs from the eager launch"
    exact = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER)
    ke = {}
    emap = exact.match(l, r, D, keep=ke)
    twin = sd.StereoMatcher(net, cv_mode=hip.MCCNN_CV_EXACT, cbca_order=hip.MCCNN_CBCA_REFERENCE_ORDER,
                            layout="plane_major")
    kt = {}
    tmap = twin.match(l, r, D, keep=kt)
    for k in ("cbca1", "sgm", "cbca2"):
        assert torch.equal(ke[k][0], kt[k][0]) and torch.equal(ke[k][1], kt[k][1]), "pixel-major %s differs" % k
    assert torch.equal(emap.view(torch.int32), tmap.view(torch.int32))
    a, b = eager.cpu().numpy(), emap.cpu().numpy()
    flips = int((kf["wta"][0] != ke["wta"][0]).sum()) + int((kf["wta"][1] != ke["wta"][1]).sum())
    close = float(np.isclose(a, b, atol=1e-3, equal_nan=True).mean())
    fin = np.isfinite(a) & np.isfinite(b)
    RECORD[cfg + "_benchmarked_fast_variant_vs_exact"] = {
        "pixels": int(a.size), "wta_flips_left_plus_right": flips, "fraction_within_1e-3_px": close,
        "max_abs_px": float(np.abs(a[fin] - b[fin]).max()),
        "abs_px_99.9th_percentile": float(np.percentile(np.abs(a[fin] - b[fin]), 99.9)), "graph_replay_equals_eager": True,
        "exact_pixel_major_equals_plane_major": True}
    _dump()
    # the stated tolerance of the fast variants (src/tolerances.py; the same constants at every configuration).
    # Round 3 measured: 0 flips at cfg2, 2 of 931 500 at cfg3, 96 of 3 000 000 at cfg4; 98.7-99.5 % within 1e-3 px
    bad = tol.fast_violations(a.size, int((kf["wta"][0] != ke["wta"][0]).sum()), int((kf["wta"][1] != ke["wta"][1]).sum()),
                              close, float(np.percentile(np.abs(np.where(fin, a - b, np.inf)), 99.0)))
    assert not bad, "%s: %s" % (cfg, "; ".join(bad))


def test_cfg3_full_size_properties():
    """KITTI-sized volume (1242x375, D=192): 6 strips per plane, 13 px of the last one; D < 256 takes the partial
    SGM kernels; the CBCA launch heuristic cuts the rows into chunks."""
    import _hipabi as hip
    import stereo_device as sd
    H, W, D = 375, 1242, 192
    g = torch.Generator(device="cuda").manual_seed(7)
    v = -torch.rand((D, H, W), device="cuda", generator=g)
    hwd = sd.dhw_to_hwd(v)
    assert torch.equal(sd.hwd_to_dhw(hwd, D), v)
    assert torch.equal(sd.wta(v), torch.argmin(v, dim=0).float())
    img = torch.rand((H, W), device="cuda", generator=g)
    img = torch.nn.functional.avg_pool2d(img[None, None], 9, 1, 4)[0, 0].contiguous()   # smooth: long arms
    sup = sd.cross_arms(img, 0.02, 14)
    assert int(sd.support_count(sup).max()) > 200
    # partition of unity + streaming vs reference-order kernel on sampled planes (incl. the first and the last)
    c = torch.full((6, H, W), -0.375, device="cuda")
    res, _ = sd.cbca(c, torch.empty_like(c), sup, 2, 14)
    assert torch.equal(res, torch.full_like(res, -0.375))
    fast, _ = sd.cbca(v.clone(), torch.empty_like(v), sup, 1, 14, hip.MCCNN_CBCA_SEPARABLE)
    idx = [0, 1, 63, 64, 100, 190, 191]
    vs = v[idx].contiguous()
    ref, _ = sd.cbca(vs.clone(), torch.empty_like(vs), sup, 1, 14, hip.MCCNN_CBCA_REFERENCE_ORDER)
    err = float((fast[idx] - ref).abs().max())
    RECORD["cfg3_streaming_vs_reference_order_max_abs"] = err
    assert err <= 8 * float(np.spacing(np.float32(1.0))), err
    # fused first pass == layout change + pass, both sides (D = 192: the partial-width kernel)
    il, ir = img, torch.rand((H, W), device="cuda", generator=g)
    vr = -torch.rand((D, H, W), device="cuda", generator=g)
    scratch = sd.sgm_scratch(H, W, D, v.device)
    hp = dict(sgm_P1=2.3, sgm_P2=55.9, sgm_Q1=4.0, sgm_Q2=8.0, sgm_D=0.08, sgm_V=1.5)
    fused = [torch.empty((H, W, sd.hwd_pitch(D)), device="cuda") for _ in range(2)]
    sd.sgm_average_from_dhw(il, ir, [v, vr], fused, [0, 1], D, scratch=scratch, **hp)
    plain = [sd.dhw_to_hwd(v), sd.dhw_to_hwd(vr)]
    sd.sgm_average_hwd(il, ir, plain, [0, 1], D, scratch=scratch, **hp)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
    # SGM shift invariance on exactly representable costs
    vi = torch.randint(0, 64, (D, H, W), device="cuda", generator=g).float()
    q = (img * 4).round() / 4
    outs = []
    for shift in (0.0, 32.0):
        h = sd.dhw_to_hwd(vi + shift)
        sd.sgm_pass_hwd(q, q, [h], [hip.MCCNN_SIDE_RIGHT], D, (0, -1), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        sd.sgm_pass_hwd(q, q, [h], [hip.MCCNN_SIDE_RIGHT], D, (1, 0), 2.0, 56.0, 4.0, 8.0, 0.08, scratch)
        outs.append(sd.hwd_to_dhw(h, D))
    assert torch.equal(outs[1], outs[0] + 32.0)
    _dump()


def test_cfg3_width_oracle_window():
    """A 1242-wide, 14-row, D=24 window through every volume stage against the CPU checker (six strips per plane, the
    last one 122 columns; row count below one row chunk)."""
    import oracle as o
    import process_functional as pf
    import synthetic
    H, W, D = 14, 1242, 24
    rng = np.random.default_rng(3)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=9)
    vl = (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    vr = (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    ol, orr = o.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 2)
    with module_setting(pf, "CBCA_ORDER", "reference"):
        gl, gr = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 2)
    assert_bits(gl, ol, "cbca reference order, W=1242")
    assert_bits(gr, orr, "cbca reference order, W=1242 (right)")
    with module_setting(pf, "CBCA_ORDER", "separable"):
        sl, sr = pf.cost_volume_aggregation(L, R, vl, vr, 0.02, 14, 2)
    assert max(np.abs(sl - ol).max(), np.abs(sr - orr).max()) <= 2 * 8 * float(np.spacing(np.float32(1.0)))
    a = o.SGM_average(ol.copy(), orr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    b = pf.SGM_average(ol.copy(), orr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    assert_bits(b[0], a[0], "SGM_average, W=1242")
    assert_bits(b[1], a[1], "SGM_average, W=1242 (right)")
    odl, odr = o.disparity_prediction(a[0], a[1])
    gdl, gdr = pf.disparity_prediction(a[0], a[1])
    assert_bits(gdl, odl, "wta W=1242")
    assert_bits(pf.interpolation(gdl, gdr, D), o.interpolation(odl, odr, D), "interpolation W=1242")


@pytest.mark.parametrize("H,W,D,kernel", [(24, 750, 256, "prog"), (20, 1242, 192, "prog"), (12, 1500, 400, "prog"),
                                          (24, 750, 256, "prog_chains"), (20, 1242, 192, "prog_chains"),
                                          (12, 1500, 400, "prog_chains"), (20, 1242, 192, "hwd")],
                         ids=["cfg2_width_and_disparities", "cfg3_width_and_disparities", "cfg4_width_and_disparities",
                              "cfg2_one_volume_chains", "cfg3_one_volume_chains", "cfg4_one_volume_chains",
                              "cfg3_width_cbca_hwd_fallback"])
def test_oracle_windows_at_real_width_and_disparity_range(H, W, D, kernel):
    """The SHIPPED default kernels against the CPU checker at the REAL width and the REAL disparity range of cfg2 / cfg3 /
    cfg4 on a window of rows: cost volume written pixel-major -> CBCA x2 -> SGM_average -> CBCA x4 -> WTA (pf:78-113,
    149-163, 187-235, 545-566, 245-254), every stage fed the GPU's own previous output.  The aggregation is what
    StereoMatcher runs at these shapes: the program-driven assembly kernels (mccnn_cbca_prog_build_pair /
    _build_skip_pair, mccnn_cbca_iter_prog_pair, and in the four-iteration aggregation two mccnn_cbca_iter_prog_pair_skip
    launches followed by mccnn_cbca_iter_prog_pair_wta where one chunk holds D) - v4 kernels at 750x256, v3 at 1242x192,
    v4 with two chunks (and WTA as its own launch) at 1500x400; one case keeps cbca_hwd_kernel, the fallback for images
    wider than a program op can index (W > 2180).  The heights sit below / at the arm limit so the vertical arms clip at
    both borders.  The `*_one_volume_chains` cases run the launches a pair really issues since round 5: the ONE-volume
    entry points mccnn_cbca_iter_prog / mccnn_cbca_iter_prog_skip, the left chain on the current stream, the right one on
    a second stream (34 of a pair's 35 aggregation launches), straight against the CPU checker."""
    import oracle as o
    import stereo_device as sd
    import synthetic
    rng = np.random.default_rng(H + W + D)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=17)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    f = rng.standard_normal((2, H, W, 64)).astype(np.float32)
    f /= np.sqrt((f * f).sum(-1, keepdims=True)).astype(np.float32)
    fl, fr = np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])
    # a2
    gl, gr = sd.cost_volume_hwd(dev(fl), dev(fr), D)
    ol, orr = o.compute_cost_volume(fl, fr, D)
    cl, cr = sd.hwd_to_dhw(gl, D).cpu().numpy(), sd.hwd_to_dhw(gr, D).cpu().numpy()
    assert_bits(cl, ol, "cost volume %dx%d" % (W, D))
    assert_bits(cr, orr, "cost volume %dx%d (right)" % (W, D))
    # a4 x 2
    sl, sr = sd.cross_arms_pair(l, r, 0.02, 14)
    words = sl.cpu().numpy().view(np.uint32).reshape(-1)[:H * W]
    assert ((words & 0xfffff) == 0).any() and not ((words & 0xfffff) == 0).all()      # the skip launches have work to skip
    if kernel in ("prog", "prog_chains"):
        progs = sd.cbca_prog_buffers(D, H, W, l.device)
        assert progs is not None
        sd.cbca_prog_build_pair(sl, sr, D, 14, progs)
        chains = dict(right_stream=sd.right_stream(l.device)) if kernel == "prog_chains" else {}

        def aggregate(a, ta, b, tb, n, **kw):
            return sd.cbca_prog_pair(a, ta, sl, b, tb, sr, progs, D, n, 14, **dict(kw, **chains))
    else:
        def aggregate(a, ta, b, tb, n, **kw):
            return sd.cbca_hwd_pair(a, ta, sl, b, tb, sr, D, n, 14, **kw)
    (gl, tl), (gr, tr) = aggregate(gl, torch.full_like(gl, float("nan")), gr, torch.full_like(gr, float("nan")), 2)
    ol, orr = o.cost_volume_aggregation(L, R, cl, cr, 0.02, 14, 2)
    cl, cr = sd.hwd_to_dhw(gl, D).cpu().numpy(), sd.hwd_to_dhw(gr, D).cpu().numpy()
    assert_bits(cl, ol, "CBCA x2 %dx%d" % (W, D))
    assert_bits(cr, orr, "CBCA x2 %dx%d (right)" % (W, D))
    # a5 / a6
    scratch = sd.sgm_scratch(H, W, D, l.device)
    sd.sgm_average_hwd(l, r, [gl, gr], [0, 1], D, 2.3, 55.9, 4.0, 8.0, 0.08, 1.5, scratch)
    ol, orr = o.SGM_average(cl.copy(), cr.copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    cl, cr = sd.hwd_to_dhw(gl, D).cpu().numpy(), sd.hwd_to_dhw(gr, D).cpu().numpy()
    assert_bits(cl, ol, "SGM_average %dx%d" % (W, D))
    assert_bits(cr, orr, "SGM_average %dx%d (right)" % (W, D))
    # a4 again: four iterations (full, skip, skip, full + WTA where one chunk holds D) keep the checker in seconds
    fused = D <= sd.cbca_hwd_wta_max_d()
    wl, wr = torch.empty((H, W), device="cuda"), torch.empty((H, W), device="cuda")
    tl.fill_(float("nan"))
    tr.fill_(float("nan"))
    (gl, _), (gr, _) = aggregate(gl, tl, gr, tr, 4, wta_out=(wl, wr) if fused else None)
    if not fused:
        wl, wr = sd.wta_hwd(gl, D), sd.wta_hwd(gr, D)
    ol, orr = o.cost_volume_aggregation(L, R, cl, cr, 0.02, 14, 4)
    assert_bits(sd.hwd_to_dhw(gl, D).cpu().numpy(), ol, "CBCA x4 %dx%d" % (W, D))
    assert_bits(sd.hwd_to_dhw(gr, D).cpu().numpy(), orr, "CBCA x4 %dx%d (right)" % (W, D))
    # a7
    odl, odr = o.disparity_prediction(ol, orr)
    assert_bits(wl.cpu().numpy(), odl, "WTA %dx%d" % (W, D))
    assert_bits(wr.cpu().numpy(), odr, "WTA %dx%d (right)" % (W, D))


def test_sgm_infinite_costs_match_the_oracle():
    """pf:545-566 with +inf costs scattered through both volumes (never a whole disparity vector): Python's min and
    np.amin treat them like the kernel's v_min_f32 / v_min3_f32, every direction and side bit-exact.  NaN and -inf costs
    are outside the kernel's contract (np.amin would turn the rest of the scanline into NaN, v_min_f32 drops a NaN
    operand): INTEGRATION.md "Limits"."""
    import oracle as o
    import stereo_device as sd
    import synthetic
    H, W, D = 23, 61, 40
    rng = np.random.default_rng(5)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=21)
    vols = []
    for _ in range(2):
        v = (rng.random((D, H, W), dtype=np.float32) * 4 - 2).astype(np.float32)
        v[rng.random((D, H, W)) < 0.02] = np.inf
        v[0][np.isinf(v).all(axis=0)] = 1.0
        vols.append(v)
    want = o.SGM_average(vols[0].copy(), vols[1].copy(), L, R, 2.3, 55.9, 4, 8, 0.08, 1.5)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    hw = [sd.dhw_to_hwd(dev(v)) for v in vols]
    sd.sgm_average_hwd(l, r, hw, [0, 1], D, 2.3, 55.9, 4.0, 8.0, 0.08, 1.5, sd.sgm_scratch(H, W, D, l.device))
    assert np.isinf(want[0]).any() and not np.isnan(want[0]).all()
    assert_bits(sd.hwd_to_dhw(hw[0], D).cpu().numpy(), want[0], "SGM_average with +inf costs (left)")
    assert_bits(sd.hwd_to_dhw(hw[1], D).cpu().numpy(), want[1], "SGM_average with +inf costs (right)")


def test_feature_row_tiling_matches_untiled_and_cfg4_memory(net_layers):
    """NET.features_pair_hwc(tile_rows=...) against the untiled stack (same receptive fields; MIOpen may
    pick another algorithm for another shape, hence a tolerance), and the peak device memory of the feature stage at
    cfg4 (1500x1000) untiled vs tiled - the number that decides whether tiling is ever needed on a 288 GB part."""
    import synthetic
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    L, R, _, _, _ = synthetic.make_pair(150, 220, 16, seed=2)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    a = net.features_pair_hwc(l, r)
    for rows in (37, 64, 150):
        b = net.features_pair_hwc(l, r, tile_rows=rows)
        err = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
        assert err <= 2e-6, (rows, err)
    H, W = 1000, 1500
    g = torch.Generator(device="cuda").manual_seed(0)
    l, r = torch.randn((H, W), device="cuda", generator=g), torch.randn((H, W), device="cuda", generator=g)
    peaks = {}
    for name, rows in (("untiled", None), ("tile_rows_125", 125)):
        net.features_pair_hwc(l, r, tile_rows=rows)              # warm-up: MIOpen picks its kernels
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f = net.features_pair_hwc(l, r, tile_rows=rows)
        torch.cuda.synchronize()
        peaks[name] = int(torch.cuda.max_memory_allocated() - base)
        del f
    RECORD["cfg4_feature_stage_peak_bytes"] = peaks
    _dump()
    assert peaks["tile_rows_125"] < peaks["untiled"]
    assert peaks["untiled"] < 16 * 2 ** 30                       # far below 288 GB: tiling stays optional
