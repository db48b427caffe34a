"""GPU: the NumPy drop-in (process_functional) at the edges of check_envelope - the reduced grid of envelope_grid.py,
stage by stage under the module defaults, every stage fed the ORACLE's previous output so that a difference stays in its
own stage, every output bit for bit."""
import numpy as np
import pytest

import envelope_grid as grid
from helpers import Tally, module_setting

pytestmark = pytest.mark.gpu

DIRS = dict(right=(0, 1), left=(0, -1), up=(-1, 0), bottom=(1, 0))
_CHAINS = {}


@pytest.fixture(scope="module")
def pf():
    import _hipabi
    _hipabi.require_device()
    import process_functional
    assert (process_functional.COST_VOLUME_MODE, process_functional.CBCA_ORDER) == ("exact", "reference")
    return process_functional


@pytest.fixture(scope="module")
def o():
    import oracle
    return oracle


def _chain(o, shape):
    """The oracle's chain of a grid shape from seeded unit features: (left, right, features, hyper-parameters, stages).
    Computed once and shared; the tests hand out copies wherever a stage writes to its arguments."""
    if shape not in _CHAINS:
        L, R = grid.make_pair(shape)
        fl, fr = grid.unit_features(shape)
        final, st = o.match_from_features(L, R, fl, fr, shape[2], return_all=True)
        for stage, res in st.items():
            for a in (res if isinstance(res, tuple) else (res,)):
                assert np.isfinite(a).all(), "%s: the oracle's %s is not finite" % (grid.name(shape), stage)
        _CHAINS[shape] = (L, R, (fl, fr), dict(o.MATCH_DEFAULTS), st)
    return _CHAINS[shape]


def _pair(t, got, want, what):
    t.bits(got[0], want[0], what + ", left")
    t.bits(got[1], want[1], what + ", right")


def test_dropin_cost_volume_and_aggregation(pf, o):
    """compute_cost_volume; cost_volume_aggregation with 2 and then 16 iterations, under the default order (the
    aggregation programs) and under the plane-major reference order; the arguments stay as they were."""
    t = Tally("drop-in volumes")
    for shape in grid.REDUCED:
        what = grid.name(shape)
        L, R, (fl, fr), hp, st = _chain(o, shape)
        tau, dist = hp["cbca_intensity"], hp["cbca_distance"]
        _pair(t, pf.compute_cost_volume(fl, fr, shape[2]), st["cost_volume"], what + ": cost volume")
        for order in ("reference", "reference_plane_major"):
            with module_setting(pf, "CBCA_ORDER", order):
                for src, n, dst in (("cost_volume", hp["cbca_num_iterations1"], "cbca1"),
                                    ("sgm", hp["cbca_num_iterations2"], "cbca2")):
                    a, b = st[src][0].copy(), st[src][1].copy()
                    _pair(t, pf.cost_volume_aggregation(L, R, a, b, tau, dist, n), st[dst],
                          "%s: aggregation x%d, CBCA_ORDER=%s" % (what, n, order))
                    _pair(t, (a, b), st[src], "%s: aggregation x%d, CBCA_ORDER=%s, arguments" % (what, n, order))
    t.settle(floor=len(grid.REDUCED) * (2 + 2 * 2 * 4))


def test_dropin_sgm(pf, o):
    """SGM_average - its result and the reference's mutation of its arguments - and the four semi_global_matching
    directions on both sides (in place, the argument handed back)."""
    t = Tally("drop-in SGM")
    for shape in grid.REDUCED:
        what = grid.name(shape)
        L, R, _, hp, st = _chain(o, shape)
        sgm = [hp[k] for k in ("sgm_P1", "sgm_P2", "sgm_Q1", "sgm_Q2", "sgm_D", "sgm_V")]
        a, b = st["cbca1"][0].copy(), st["cbca1"][1].copy()
        wa, wb = st["cbca1"][0].copy(), st["cbca1"][1].copy()
        want = o.SGM_average(wa, wb, L, R, *sgm)
        _pair(t, want, st["sgm"], what + ": the oracle's SGM_average against its own chain")
        _pair(t, pf.SGM_average(a, b, L, R, *sgm), want, what + ": SGM_average")
        _pair(t, (a, b), (wa, wb), what + ": SGM_average, arguments afterwards")
        for dname, r in DIRS.items():
            p1 = hp["sgm_P1"] if r[0] == 0 else hp["sgm_P1"] / hp["sgm_V"]
            args = (p1, hp["sgm_P2"], hp["sgm_Q1"], hp["sgm_Q2"], hp["sgm_D"])
            for side, choice in enumerate("LR"):
                v, w = st["cbca1"][side].copy(), st["cbca1"][side].copy()
                out = pf.semi_global_matching(L, R, v, r, *args, choice)
                t.check(out is v, "%s: semi_global_matching %s %s hands back another array" % (what, dname, choice))
                t.bits(v, o.semi_global_matching(L, R, w, r, *args, choice),
                       "%s: semi_global_matching %s %s" % (what, dname, choice))
    t.settle(floor=len(grid.REDUCED) * (6 + 4 * 2 * 2))


def test_dropin_maps(pf, o):
    """disparity_prediction, interpolation, subpixel_enhance, median_filter(5, 5) and bilateral_filter."""
    t = Tally("drop-in maps")
    for shape in grid.REDUCED:
        what = grid.name(shape)
        L, R, _, hp, st = _chain(o, shape)
        D = shape[2]
        _pair(t, pf.disparity_prediction(*st["cbca2"]), st["wta"], what + ": disparity_prediction")
        t.bits(pf.interpolation(st["wta"][0], st["wta"][1], D), st["interp"], what + ": interpolation")
        t.bits(pf.subpixel_enhance(st["interp"], st["cbca2"][0]), st["subpixel"], what + ": subpixel_enhance")
        t.bits(pf.median_filter(st["subpixel"], 5, 5), st["median"], what + ": median_filter")
        t.bits(pf.bilateral_filter(L, st["median"], 5, 5, 0, hp["blur_sigma"], hp["blur_threshold"]), st["bilateral"],
               what + ": bilateral_filter")
    t.settle(floor=len(grid.REDUCED) * 6)


def test_dropin_cross_regions(pf, o):
    """compute_cross_region with the grid's distances 14 and 28: the lists and the counts of both images."""
    t = Tally("drop-in cross regions")
    for shape in grid.REDUCED:
        L, R, _, hp, _ = _chain(o, shape)
        for dist in grid.DISTANCES:
            for img, side in ((L, "left"), (R, "right")):
                what = "%s: compute_cross_region, distance %d, %s" % (grid.name(shape), dist, side)
                region, num = pf.compute_cross_region(img, hp["cbca_intensity"], dist)
                want_region, want_num = o.compute_cross_region(img, hp["cbca_intensity"], dist)
                t.equal(region, want_region, what + ": lists")
                t.equal(num, want_num, what + ": counts")
    t.settle(floor=len(grid.REDUCED) * len(grid.DISTANCES) * 2 * 2)
