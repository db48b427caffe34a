"""GPU: every kernel route against the REFERENCE's own recorded outputs (tests/golden/route_*.npz, made by
tests/golden/gen_route_golden.py), bit for bit through helpers.Tally (bits_strict).  Only fixtures are read - never the reference,
never the CPU oracle's arithmetic (test_reference_routes_cpu.py pins the oracle to the same files).  Only the bit-exact
variants run: MCCNN_CV_EXACT and MCCNN_CBCA_REFERENCE_ORDER; there is no tolerance anywhere.

fixture family -> routes
  route_sgm_*   mccnn_sgm_pass (both volumes in one launch, and one launch per volume), mccnn_sgm_flags +
                mccnn_sgm_pass_flagged, sgm_average_hwd, sgm_average_from_dhw (mccnn_sgm_first_pass up to D = 256, the
                separate layout change above), mccnn_sgm_pass_accumulate in its three modes and as the paper's four-pass
                chain.  D = 5 .. 1024 cover the ten near classes of sgm_route() (asserted).  The far routes (volumes past
                4 GiB) cannot be reached by a fixture; test_large_volume_gpu.py compares them with crops.  The files at
                D = 192, 256 and D >= 512 hold exact sums (dyadic penalties): they pin groups, tail masks and the minimum
                across groups; the order of additions shows at D = 5, 130, 257 and in the W > D pair.
  route_cbca_*  cross_arms, cross_arms_pair, cross_region_list; plane-major cbca_pair in reference order; cbca_hwd_pair
                (mccnn_cbca_iter_hwd_pair up to distance 14, mccnn_cbca_iter_hwd_long_pair from 15); cbca_prog_pair as
                two-volume launches and as one-volume chains (full and skip programs), a refresh / skip / skip chain, and
                the fused-WTA last iteration of both families.  Distances above 14 have no programs and no fused WTA: the
                refusals are asserted.  An even number of iterations (where skip_schedule issues the refresh launch by
                itself) is not among the fixtures.
  route_cv_*    cost_volume, cost_volume_hwd (exact mode)
  route_post_*  wta / wta_hwd, lr_status + interpolate, subpixel / subpixel_hwd, median, bilateral"""
import numpy as np
import pytest
import torch

import paper_sgm_reference as paper
import route_fixtures as rf
from helpers import Tally, hp_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    import stereo_device
    return stereo_device


@pytest.fixture(scope="module")
def hip():
    import _hipabi
    return _hipabi


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # (a copy: the fixtures are read-only)


def host(t):
    return t.cpu().numpy()


# ---- SGM ----------------------------------------------------------------------------------------------------------------
def sgm_cases():
    """(case, {key: array}) with both sides: the penalty-class pair is stored as one file per side."""
    merged = {}
    for name, g in rf.family("sgm"):
        case = name[:-2] if name.startswith("route_sgm_pen") else name
        merged.setdefault(case, {}).update(g)
    return merged


def test_sgm_fixtures_cover_every_near_route_class():
    have = {rf.sgm_route(int(g["vol_l"].shape[0])) for g in sgm_cases().values()}
    assert have == rf.SGM_NEAR_CLASSES


@pytest.mark.parametrize("case", sorted(sgm_cases()))
def test_sgm_routes(sd, hip, case):
    g = sgm_cases()[case]
    hp = hp_of(g)
    pen = [hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]
    p1h, p1v, p2, q1, q2, thr = sd._sgm_penalties(*pen)
    D, H, W = g["vol_l"].shape
    l, r = dev(g["left"][:, :, 0]), dev(g["right"][:, :, 0])
    vols = [dev(g["vol_l"]), dev(g["vol_r"])]
    sides = [hip.MCCNN_SIDE_LEFT, hip.MCCNN_SIDE_RIGHT]
    scratch = sd.sgm_scratch(H, W, D, l.device)
    planes = sd.sgm_flag_planes(l, r, D, pen[4])
    t = Tally(case)

    def fresh():
        return [sd.dhw_to_hwd(v) for v in vols]

    def back(h):
        return host(sd.hwd_to_dhw(h, D))

    for i, (dname, rr) in enumerate(rf.DIRS.items()):
        assert rr == sd.SGM_DIRECTIONS[i]
        p1 = p1h if rr[0] == 0 else p1v
        want = [g["sgm_%s_%s" % (dname, s)] for s in "lr"]
        h = fresh()                                                     # both volumes in one launch
        sd.sgm_pass_hwd(l, r, h, sides, D, rr, p1, p2, q1, q2, thr, scratch)
        for k in (0, 1):
            t.bits(back(h[k]), want[k], "%s %s side %d, one launch" % (case, dname, k))
        h = fresh()                                                     # one launch per volume
        for k in (0, 1):
            sd.sgm_pass_hwd(l, r, [h[k]], [sides[k]], D, rr, p1, p2, q1, q2, thr, scratch)
            t.bits(back(h[k]), want[k], "%s %s side %d, its own launch" % (case, dname, k))
        h = fresh()                                                     # flag planes built once
        sd.sgm_pass_flagged_hwd(h, sides, D, rr, p1, p2, q1, q2, planes[i])
        for k in (0, 1):
            t.bits(back(h[k]), want[k], "%s %s side %d, flagged" % (case, dname, k))
        # the accumulating form: store, add, add and quarter (what the accumulator held: the other side's input)
        for k in (0, 1):
            had = g["vol_" + "rl"[k]]
            with np.errstate(invalid="ignore", over="ignore"):
                wants = {hip.MCCNN_SGM_ACC_STORE: want[k], hip.MCCNN_SGM_ACC_ADD: had + want[k],
                         hip.MCCNN_SGM_ACC_ADD_QUARTER: (had + want[k]) / np.float32(4.)}
            src = sd.dhw_to_hwd(vols[k])
            for mode, w in wants.items():
                acc = sd.dhw_to_hwd(dev(had))
                sd.sgm_pass_accumulate_hwd([src], [acc], [sides[k]], D, rr, p1, p2, q1, q2, mode, planes[i])
                t.bits(back(acc), w, "%s %s side %d, accumulate mode %d" % (case, dname, k, mode))
            t.bits(back(src), g["vol_" + "lr"[k]], "%s %s side %d: the accumulating pass wrote its source" % (case, dname, k))

    want_avg = [g["avg_l"], g["avg_r"]]
    h = fresh()
    sd.sgm_average_hwd(l, r, h, sides, D, *pen, scratch)
    for k in (0, 1):
        t.bits(back(h[k]), want_avg[k], "%s sgm_average_hwd side %d" % (case, k))
    h = fresh()
    sd.sgm_average_hwd(l, r, h, sides, D, *pen, scratch, flags=planes)
    for k in (0, 1):
        t.bits(back(h[k]), want_avg[k], "%s sgm_average_hwd with flag planes side %d" % (case, k))
    h = [torch.empty((H, W, sd.hwd_pitch(D)), dtype=torch.float32, device=l.device) for _ in (0, 1)]
    sd.sgm_average_from_dhw(l, r, [v.clone() for v in vols], h, sides, D, *pen, scratch)
    for k in (0, 1):
        t.bits(back(h[k]), want_avg[k], "%s sgm_average_from_dhw side %d" % (case, k))
    # the paper's stage: the helper's average of the reference's four single-direction outputs
    src = fresh()
    spare = [torch.full_like(s, float("nan")) for s in src]
    res, _ = sd.sgm_average_independent_hwd(l, r, src, spare, sides, D, *pen, scratch, flags=planes)
    for k, s in enumerate("lr"):
        t.bits(back(res[k]), paper.average4([g["sgm_%s_%s" % (d, s)] for d in paper.NAMES]),
               "%s independent directions side %d" % (case, k))
    t.settle()


# ---- cross regions and aggregation --------------------------------------------------------------------------------------
def region_counts(region):
    return (region[..., 0] >= 0).sum(-1).astype(np.int32)


@pytest.mark.parametrize("name", rf.names("cbca"))
def test_cross_regions(sd, name):
    g = rf.fixture(name)
    tau = hp_of(g)["cbca_intensity"]
    l, r = dev(g["left"][:, :, 0]), dev(g["right"][:, :, 0])
    t = Tally(name)
    for dist in sorted({d for d, _ in rf.cbca_cases(g)}):
        pair = sd.cross_arms_pair(l, r, tau, dist)
        for k, (s, img) in enumerate((("l", l), ("r", r))):
            for how, sup in (("cross_arms", sd.cross_arms(img, tau, dist)), ("cross_arms_pair", pair[k])):
                what = "%s %s L=%d %s" % (name, s, dist, how)
                t.equal(host(sd.support_arms(sup)), g["arms_%s_L%d" % (s, dist)], what + " arms")
                t.equal(host(sd.support_count(sup)), g["num_%s_L%d" % (s, dist)], what + " counts")
            region = host(sd.cross_region_list(pair[k], dist))
            t.equal(region_counts(region), g["num_%s_L%d" % (s, dist)], "%s %s L=%d region list counts" % (name, s, dist))
            # every entry lies inside the stored arms: rows h - up .. h + down, and on row q columns w - left(q) .. w + right(q)
            arms = g["arms_%s_L%d" % (s, dist)].astype(np.int64)
            H, W = arms.shape[:2]
            hh, ww = np.arange(H)[:, None, None], np.arange(W)[None, :, None]
            q, c = region[..., 0].astype(np.int64), region[..., 1].astype(np.int64)
            valid = q >= 0
            qc = np.clip(q, 0, H - 1)
            inside = (q >= hh - arms[:, :, None, 0]) & (q <= hh + arms[:, :, None, 1]) & \
                (c >= ww - arms[qc, ww, 2]) & (c <= ww + arms[qc, ww, 3])
            t.check(bool((inside | ~valid).all()) and bool(((q == -1) == (c == -1)).all()),
                    "%s %s L=%d: a region list entry outside the stored arms" % (name, s, dist))
    t.settle()


def aggregate_all(sd, hip, t, what, g, vl, vr, dist, its, want, want_wta):
    """Every aggregation route that serves (distance, iterations) on one volume pair."""
    tau = hp_of(g)["cbca_intensity"]
    D, H, W = vl.shape
    l, r = dev(g["left"][:, :, 0]), dev(g["right"][:, :, 0])
    sl, sr = sd.cross_arms_pair(l, r, tau, dist)
    dl, dr = dev(vl), dev(vr)

    def hwd():
        a, b = sd.dhw_to_hwd(dl), sd.dhw_to_hwd(dr)
        return a, torch.full_like(a, float("nan")), b, torch.full_like(b, -9.0)

    def check(res, how):
        (a, _), (b, _) = res
        t.bits(host(sd.hwd_to_dhw(a, D)), want[0], "%s %s left" % (what, how))
        t.bits(host(sd.hwd_to_dhw(b, D)), want[1], "%s %s right" % (what, how))

    def check_wta(out, how):
        if want_wta is not None:
            t.bits(host(out[0]), want_wta[0], "%s %s WTA left" % (what, how))
            t.bits(host(out[1]), want_wta[1], "%s %s WTA right" % (what, how))

    def wta_out():
        return (torch.full((H, W), -7.0, device=l.device), torch.full((H, W), -7.0, device=l.device))

    # plane-major, reference order
    (a, _), (b, _) = sd.cbca_pair(dl.clone(), torch.empty_like(dl), sl, dr.clone(), torch.empty_like(dr), sr, its, dist,
                                  hip.MCCNN_CBCA_REFERENCE_ORDER)
    t.bits(host(a), want[0], what + " plane-major left")
    t.bits(host(b), want[1], what + " plane-major right")
    # pixel-major: mccnn_cbca_iter_hwd_pair / mccnn_cbca_iter_hwd_long_pair
    assert sd.aggregation_route(dist, W, D, H=H, cbca_kernel="hwd") == ("hwd" if dist <= 14 else "hwd_long")
    hl, tl, hr, tr = hwd()
    check(sd.cbca_hwd_pair(hl, tl, sl, hr, tr, sr, D, its, dist), "cbca_hwd_pair")
    if dist > sd.CBCA_HWD_MAX_DISTANCE:
        # no fused WTA and no programs above distance 14: refused, not skipped
        hl, tl, hr, tr = hwd()
        with pytest.raises(ValueError, match="fused WTA"):
            sd.cbca_hwd_pair(hl, tl, sl, hr, tr, sr, D, its, dist, wta_out=wta_out())
        progs = sd.cbca_prog_buffers(D, H, W, l.device)
        with pytest.raises(hip.MccnnHipError):
            sd.cbca_prog_build_pair(sl, sr, D, dist, progs)
        return
    assert sd.aggregation_route(dist, W, D, H=H) == "prog"
    out = wta_out()
    hl, tl, hr, tr = hwd()
    check(sd.cbca_hwd_pair(hl, tl, sl, hr, tr, sr, D, its, dist, wta_out=out), "cbca_hwd_pair with the fused WTA")
    check_wta(out, "cbca_hwd_pair")
    progs = sd.cbca_prog_buffers(D, H, W, l.device)
    assert progs is not None
    sd.cbca_prog_build_pair(sl, sr, D, dist, progs)
    hl, tl, hr, tr = hwd()
    check(sd.cbca_prog_pair(hl, tl, sl, hr, tr, sr, progs, D, its, dist), "cbca_prog_pair, two-volume launches")
    hl, tl, hr, tr = hwd()
    check(sd.cbca_prog_pair(hl, tl, sl, hr, tr, sr, progs, D, its, dist, right_stream=sd.right_stream(l.device)),
          "cbca_prog_pair, one-volume chains")
    torch.cuda.synchronize()
    out = wta_out()
    hl, tl, hr, tr = hwd()
    check(sd.cbca_prog_pair(hl, tl, sl, hr, tr, sr, progs, D, its, dist, wta_out=out), "cbca_prog_pair with the fused WTA")
    check_wta(out, "cbca_prog_pair")
    if its == 3:
        assert sd.skip_schedule(3, False) == ["full", "skip", "skip"]
        # the refresh launch (the full programs, which also write v1 back at unit-region pixels) in front of two skips
        hl, tl, hr, tr = hwd()
        left, right = [hl, tl, sl, progs[0]], [hr, tr, sr, progs[1]]
        for kind in ("refresh", "skip", "skip"):
            sd._prog_launch(kind, (tuple(left), tuple(right)), D, dist, sd._NO_TIMER)
            left[0], left[1], right[0], right[1] = left[1], left[0], right[1], right[0]
        check(((left[0], None), (right[0], None)), "refresh, skip, skip (two-volume launches)")
        hl, tl, hr, tr = hwd()
        for k, vol in enumerate(([hl, tl, sl, progs[0]], [hr, tr, sr, progs[1]])):
            for kind in ("refresh", "skip", "skip"):
                sd._prog_launch(kind, (tuple(vol),), D, dist, sd._NO_TIMER)
                vol[0], vol[1] = vol[1], vol[0]
            t.bits(host(sd.hwd_to_dhw(vol[0], D)), want[k], "%s refresh, skip, skip (one-volume launches) side %d" % (what, k))


@pytest.mark.parametrize("name", rf.names("cbca"))
def test_aggregation_routes(sd, hip, name):
    g = rf.fixture(name)
    t = Tally(name)
    for dist, its in rf.cbca_cases(g):
        key = "L%d_it%d" % (dist, its)
        aggregate_all(sd, hip, t, "%s %s" % (name, key), g, g["vol_l"], g["vol_r"], dist, its,
                      (g["agg_l_" + key], g["agg_r_" + key]), (g["wta_l_" + key], g["wta_r_" + key]))
    if "special_vol_l" in g:
        for its in (1, 3):
            aggregate_all(sd, hip, t, "%s special x%d" % (name, its), g, g["special_vol_l"], g["special_vol_r"],
                          int(g["special_distance"]), its, (g["special_agg_l_it%d" % its], g["special_agg_r_it%d" % its]),
                          None)
    t.settle()


# ---- cost volume --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rf.names("cv"))
def test_cost_volume_routes(sd, hip, name):
    g = rf.fixture(name)
    D = g["cv_l" if "cv_l" in g else "cv_r"].shape[0]
    fl, fr = dev(g["fl"]), dev(g["fr"])
    t = Tally(name)
    pl, pr = sd.cost_volume(fl, fr, D, mode=hip.MCCNN_CV_EXACT)
    hl, hr = sd.cost_volume_hwd(fl, fr, D, mode=hip.MCCNN_CV_EXACT)
    for s, plane, pixel in (("l", pl, hl), ("r", pr, hr)):
        if "cv_" + s in g:
            t.bits(host(plane), g["cv_" + s], "%s cost_volume %s" % (name, s))
            t.bits(host(sd.hwd_to_dhw(pixel, D)), g["cv_" + s], "%s cost_volume_hwd %s" % (name, s))
    t.settle()


# ---- WTA .. bilateral ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rf.names("post"))
def test_post_routes(sd, name):
    g = rf.fixture(name)
    D = g["vol_l"].shape[0]
    t = Tally(name)
    img = dev(g["left"][:, :, 0])
    for s in "lr":
        v = dev(g["vol_" + s])
        t.bits(host(sd.wta(v)), g["wta_" + s], "%s wta %s" % (name, s))
        t.bits(host(sd.wta_hwd(sd.dhw_to_hwd(v), D)), g["wta_" + s], "%s wta_hwd %s" % (name, s))
    status = sd.lr_status(dev(g["wta_l"]), dev(g["wta_r"]), D)
    t.bits(host(sd.interpolate(dev(g["wta_l"]), status)), g["interp"], name + " lr_status + interpolate")
    vl = dev(g["vol_l"])
    t.bits(host(sd.subpixel(dev(g["interp"]), vl)), g["subpixel"], name + " subpixel")
    t.bits(host(sd.subpixel_hwd(dev(g["interp"]), sd.dhw_to_hwd(vl), D)), g["subpixel"], name + " subpixel_hwd")
    for fh, fw in rf.POST_WINDOWS:
        t.bits(host(sd.median(dev(g["subpixel"]), fh, fw)), g["median_%dx%d" % (fh, fw)], "%s median %dx%d" % (name, fh, fw))
    for sigma, thr in rf.POST_BILATERAL:
        t.bits(host(sd.bilateral(img, dev(g["median_5x5"]), 5, 5, 0, sigma, thr)), g["bilateral_s%g_t%g" % (sigma, thr)],
               "%s bilateral sigma %g threshold %g" % (name, sigma, thr))
    t.settle()
