"""CPU: the C oracle (oracle/mccnn_oracle.c) against tests/golden/route_*.npz - the reference's own outputs at the shapes
where the kernel routes part (tests/golden/gen_route_golden.py) - bit for bit.  Needs no reference: it also runs where
test_oracle_vs_reference_cpu.py skips.  test_reference_routes_gpu.py compares every kernel route with the same files."""
import numpy as np
import pytest

import oracle as o
import paper_sgm_reference as paper
import route_fixtures as rf
from helpers import Tally, assert_bits, hp_of


def test_sgm_fixtures_cover_every_near_route_class():
    have = {rf.sgm_route(int(g["vol_" + rf.sgm_sides(g)[0]].shape[0])) for _, g in rf.family("sgm")}
    assert have == rf.SGM_NEAR_CLASSES
    assert [rf.sgm_route(D) for D in rf.SGM_CLASSES] == [
        (1, False, 4), (1, False, 3), (1, True, 3), (1, True, 4), (2, False, 4), (2, True, 4), (3, False, 4), (3, True, 4),
        (4, False, 4), (4, True, 4)]


@pytest.mark.parametrize("name", rf.names("sgm"))
def test_sgm(name):
    g = rf.fixture(name)
    hp = hp_of(g)
    t = Tally(name)
    L, R = g["left"], g["right"]
    pen = [hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]
    for s in rf.sgm_sides(g):
        ch = s.upper()
        for dname, r in rf.DIRS.items():
            v = g["vol_" + s].copy()
            p1 = hp["sgm_P1"] if r[0] == 0 else hp["sgm_P1"] / hp["sgm_V"]
            o.semi_global_matching(L, R, v, r, p1, hp["sgm_P2"], hp["sgm_Q1"], hp["sgm_Q2"], hp["sgm_D"], ch)
            t.bits(v, g["sgm_%s_%s" % (dname, s)], "%s %s %s" % (name, dname, ch))
        # the independent-directions stage: the helper's average of the reference's four stored outputs
        want = paper.average4([g["sgm_%s_%s" % (d, s)] for d in paper.NAMES])
        t.bits(paper.sgm_independent(g["vol_" + s], L, R, *pen, ch), want, "%s independent %s" % (name, ch))
    vols = {s: g["vol_" + s].copy() for s in rf.sgm_sides(g)}
    other = np.zeros_like(next(iter(vols.values())))
    al, ar = o.SGM_average(vols.get("l", other), vols.get("r", other), L, R, *pen)
    for s, a in (("l", al), ("r", ar)):
        if s in vols:
            t.bits(a, g["avg_" + s], "%s SGM_average %s" % (name, s))
    t.settle()


@pytest.mark.parametrize("name", rf.names("cbca"))
def test_cross_regions_and_aggregation(name):
    g = rf.fixture(name)
    tau = hp_of(g)["cbca_intensity"]
    t = Tally(name)
    L, R = g["left"], g["right"]
    for dist in sorted({d for d, _ in rf.cbca_cases(g)}):
        for s, img in (("l", L), ("r", R)):
            arms, cnt = o.cross_arms(img, tau, dist)
            t.equal(arms, g["arms_%s_L%d" % (s, dist)], "%s arms %s L=%d" % (name, s, dist))
            t.equal(cnt, g["num_%s_L%d" % (s, dist)], "%s counts %s L=%d" % (name, s, dist))
            _reg, num = o.compute_cross_region(img, tau, dist)
            t.equal(num, g["num_%s_L%d" % (s, dist)], "%s region counts %s L=%d" % (name, s, dist))
    for dist, its in rf.cbca_cases(g):
        key = "L%d_it%d" % (dist, its)
        al, ar = o.cost_volume_aggregation(L, R, g["vol_l"], g["vol_r"], tau, dist, its)
        t.bits(al, g["agg_l_" + key], "%s agg l %s" % (name, key))
        t.bits(ar, g["agg_r_" + key], "%s agg r %s" % (name, key))
        dl, dr = o.disparity_prediction(g["agg_l_" + key], g["agg_r_" + key])
        t.bits(dl, g["wta_l_" + key], "%s wta l %s" % (name, key))
        t.bits(dr, g["wta_r_" + key], "%s wta r %s" % (name, key))
    if "special_vol_l" in g:
        dist = int(g["special_distance"])
        for its in (1, 3):
            al, ar = o.cost_volume_aggregation(L, R, g["special_vol_l"], g["special_vol_r"], tau, dist, its)
            t.bits(al, g["special_agg_l_it%d" % its], "%s special l it=%d" % (name, its))
            t.bits(ar, g["special_agg_r_it%d" % its], "%s special r it=%d" % (name, its))
    t.settle()


@pytest.mark.parametrize("name", rf.names("cv"))
def test_cost_volume(name):
    g = rf.fixture(name)
    key = "cv_l" if "cv_l" in g else "cv_r"
    with np.errstate(all="ignore"):
        l, r = o.compute_cost_volume(g["fl"], g["fr"], g[key].shape[0])
    if "cv_l" in g:
        assert_bits(l, g["cv_l"], name + " cv_l")
    if "cv_r" in g:
        assert_bits(r, g["cv_r"], name + " cv_r")


@pytest.mark.parametrize("name", rf.names("post"))
def test_wta_to_bilateral(name):
    g = rf.fixture(name)
    D = g["vol_l"].shape[0]
    t = Tally(name)
    dl, dr = o.disparity_prediction(g["vol_l"], g["vol_r"])
    t.bits(dl, g["wta_l"], name + " wta_l")
    t.bits(dr, g["wta_r"], name + " wta_r")
    t.bits(o.interpolation(g["wta_l"], g["wta_r"], D), g["interp"], name + " interp")
    t.bits(o.subpixel_enhance(g["interp"], g["vol_l"]), g["subpixel"], name + " subpixel")
    for fh, fw in rf.POST_WINDOWS:
        t.bits(o.median_filter(g["subpixel"], fh, fw), g["median_%dx%d" % (fh, fw)], "%s median %dx%d" % (name, fh, fw))
    for sigma, thr in rf.POST_BILATERAL:
        t.bits(o.bilateral_filter(g["left"], g["median_5x5"], 5, 5, 0, sigma, thr), g["bilateral_s%g_t%g" % (sigma, thr)],
               "%s bilateral %g %g" % (name, sigma, thr))
    t.settle()
