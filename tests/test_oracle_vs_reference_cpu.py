"""CPU, development container only: the C oracle (oracle/mccnn_oracle.c) against the reference itself, run live through
tests/golden/ref_shim.py, stage by stage and bit for bit (helpers.bits_strict for float32; np.array_equal plus dtype for
integers).  Where the reference is absent - the GPU machine, a checkout elsewhere - the whole module skips;
test_reference_routes_cpu.py then still pins the oracle to the reference's recorded outputs.

Matrix: five kinds of image (smooth pair, constant, vertical bands, integer levels * float32(0.02), Gaussian noise) at
(H, W, D) = (9,17,5), (6,40,33), (31,12,3), (1,9,2), (3,3,2); every stage's own settings are listed at its test.  Every case
is compared; failures are collected per stage and reported together (settle), and every stage prints the number of
comparisons it made and asserts it against a floor (FLOORS: the counts of the first run), so a matrix that shrinks fails.

The W > D >= 130 SGM case is (6,140,130), where one reference pass takes about 3 s: it runs on the levels pair only -
the four directions on both sides at the default penalties, the same at the second penalty setting with +-inf / -0.0
planted, and SGM_average at the defaults.  Every other SGM case runs all three penalty settings with and without planted
values on all five kinds of image.

The reference refuses three kinds of input that the oracle accepts (REFUSED below); they are outside its domain, not
differences.  For those the test records that the reference raised and compares nothing.  Any other exception fails.

One departure is pinned by name (test_sgm_nan_departure): a NaN cost makes the reference's np.amin over the previous line
NaN, so every cost behind it on the path is NaN; the oracle's comparisons drop it from the minimum over the line, and
only the NaN's own disparity stays NaN along the path.  A NaN on plane 0, from which the oracle's minimum starts, does
make the whole line NaN, as in the reference; that is pinned too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import ref_shim  # noqa: E402

if not ref_shim.available():
    pytest.skip("the reference sources are not on this machine (MCCNN_REFERENCE_SRC): the live differential test runs "
                "in the development container only", allow_module_level=True)

import oracle as o  # noqa: E402
from helpers import Tally, smooth_pair  # noqa: E402

KINDS = ("smooth", "constant", "bands", "levels", "noise")
SHAPES = ((9, 17, 5), (6, 40, 33), (31, 12, 3), (1, 9, 2), (3, 3, 2))
SGM_WIDE = (6, 140, 130)
DIRS = dict(right=(0, 1), left=(0, -1), up=(-1, 0), bottom=(1, 0))
CROSS = ((0.02, 14), (0.02, 1), (0.04, 28), (0.02, 20), (0.02, 32), (1e9, 32))
AGGREGATION = ((0.02, 14, 2), (0.04, 28, 1), (0.02, 3, 3))
PENALTIES = ((2.3, 55.9, 4, 8, 0.08), (1.0, 32.0, 3, 6, 0.0), (0.5, 2.0, 1, 1, 10.0))
SGM_V = 1.5
WINDOWS = ((5, 5), (3, 3), (1, 7), (7, 3), (9, 9))
BILATERAL = ((6, 2), (1, 0.5), (3, 100))
CV_SHAPES = ((5, 12, 4, 64), (3, 40, 38, 64), (2, 9, 7, 64), (4, 30, 8, 112), (2, 132, 130, 64))
# inputs the reference itself refuses: (what, the exception it raises)
REFUSED = (("intensity_threshold = 0 (pf:601: the arm test stops at the pixel itself, count = 0)", AssertionError),
           ("D = 1 in semi_global_matching (pf:550 reads plane d + 1)", IndexError),
           ("a NaN column in disparity_prediction (pf:253: no disparity wins)", AssertionError))
# comparisons per stage in the first run of this file
FLOORS = dict(cross=450, aggregation=300, sgm=1216, sgm_average=104, post=840, cost_volume=20, refused=3, nan=6)


@pytest.fixture(scope="module")
def pf():
    return ref_shim.load_reference()[0]


def image_pair(kind, H, W, seed=0):
    rng = np.random.default_rng(seed * 7919 + H * 131 + W)
    if kind == "smooth":
        a, b = (t.numpy() for t in smooth_pair(H, W, seed + 1))
    elif kind == "constant":
        a, b = np.full((H, W), 0.3), np.full((H, W), -1.25)
    elif kind == "bands":
        a = np.tile((np.arange(W) // 3 % 4) * 0.5, (H, 1))
        b = np.tile((np.arange(W) // 5 % 3) * 0.25, (H, 1))
    elif kind == "levels":
        a, b = (rng.integers(0, 4, (H, W)) * np.float32(0.02) for _ in range(2))
    else:
        a, b = rng.standard_normal((H, W)), rng.standard_normal((H, W))
    return tuple(np.ascontiguousarray(x, dtype=np.float32)[:, :, None] for x in (a, b))


def volume(rng, D, H, W, special=()):
    v = rng.uniform(-1.0, 0.0, (D, H, W)).astype(np.float32)
    if special and v.size >= 4 * len(special):
        idx = rng.choice(v.size, 2 * len(special), replace=False)
        v.reshape(-1)[idx] = np.asarray(list(special) * 2, dtype=np.float32)
    return v


def settle(t):
    print("%s: %d comparisons of the oracle with the reference" % (t.what, t.total))
    t.settle(FLOORS[t.what])


def ref(fn, *args):
    """The reference's result; its exceptions pass through (a test that expects one catches it by type)."""
    with ref_shim.quiet(), np.errstate(all="ignore"):
        return fn(*args)


# ---- a3 -----------------------------------------------------------------------------------------------------------------
def test_cross_regions(pf):
    t = Tally("cross")
    on_threshold = 0
    for kind in KINDS:
        for H, W, _ in SHAPES:
            img = image_pair(kind, H, W)[0]
            for tau, dist in CROSS:
                what = "%s %dx%d tau=%g L=%d" % (kind, H, W, tau, dist)
                want_reg, want_num = ref(pf.compute_cross_region, img, tau, dist)
                reg, num = o.compute_cross_region(img, tau, dist)
                t.equal(num, want_num, what + " counts")
                t.equal(reg, want_reg, what + " coordinate lists")
                arms, cnt = o.cross_arms(img, tau, dist)
                t.equal(cnt, want_num, what + " counts (cross_arms)")
                if kind == "levels" and tau == 0.02:
                    g = img[:, :, 0]
                    for h in range(H):
                        for w in range(W):
                            rt = int(arms[h, w, 3])
                            if rt < dist - 1 and w + rt + 1 < W:
                                assert abs(g[h, w] - g[h, w + rt + 1]) >= np.float32(tau)
                                on_threshold += int(abs(g[h, w] - g[h, w + rt + 1]) == np.float32(tau))
    assert on_threshold > 0, "no arm ends on a difference equal to the threshold: the `>=` of pf:588 is not exercised"
    settle(t)


# ---- a4 -----------------------------------------------------------------------------------------------------------------
def test_aggregation(pf):
    t = Tally("aggregation")
    for ki, kind in enumerate(KINDS):
        for H, W, D in SHAPES:
            L, R = image_pair(kind, H, W)
            rng = np.random.default_rng(ki * 100 + H)
            for special in ((), (np.nan, np.inf, -np.inf, 0.0, -0.0)):
                vl, vr = volume(rng, D, H, W, special), volume(rng, D, H, W, special)
                for tau, dist, its in AGGREGATION:
                    what = "%s %dx%dx%d tau=%g L=%d x%d%s" % (kind, H, W, D, tau, dist, its, " special" if special else "")
                    wl, wr = ref(pf.cost_volume_aggregation, L, R, vl, vr, tau, dist, its)
                    gl, gr = o.cost_volume_aggregation(L, R, vl, vr, tau, dist, its)
                    t.bits(gl, wl, what + " left")
                    t.bits(gr, wr, what + " right")
    settle(t)


# ---- a5 / a6 ------------------------------------------------------------------------------------------------------------
def sgm_single(pf, t, L, R, vol, pen, what):
    p1, p2, q1, q2, thr = pen
    for dname, r in DIRS.items():
        for ch in "LR":
            p1r = p1 if r[0] == 0 else p1 / SGM_V
            want = ref(pf.semi_global_matching, L, R, vol.copy(), r, p1r, p2, q1, q2, thr, ch)
            got = o.semi_global_matching(L, R, vol.copy(), r, p1r, p2, q1, q2, thr, ch)
            t.bits(got, want, "%s %s %s" % (what, dname, ch))


def wide_pair():
    """W > D >= 130: the levels pair, in steps of 0.06 so that both sides of sgm_D = 0.08 occur."""
    L, R = image_pair("levels", SGM_WIDE[0], SGM_WIDE[1])
    return L * np.float32(3), R * np.float32(3)


def test_sgm_single_directions(pf):
    t = Tally("sgm")
    for ki, kind in enumerate(KINDS):
        for H, W, D in SHAPES:
            L, R = image_pair(kind, H, W)
            rng = np.random.default_rng(ki * 100 + W)
            for pi, pen in enumerate(PENALTIES):
                for special in ((), (np.inf, -np.inf, -0.0)):
                    vol = volume(rng, D, H, W, special)
                    sgm_single(pf, t, L, R, vol, pen, "%s %dx%dx%d pen %d%s" % (kind, H, W, D, pi, " special" if special
                                                                                  else ""))
    L, R = wide_pair()
    H, W, D = SGM_WIDE
    rng = np.random.default_rng(1)
    sgm_single(pf, t, L, R, volume(rng, D, H, W), PENALTIES[0], "levels %dx%dx%d pen 0" % SGM_WIDE)
    sgm_single(pf, t, L, R, volume(rng, D, H, W, (np.inf, -np.inf, -0.0)), PENALTIES[1],
               "levels %dx%dx%d pen 1 special" % SGM_WIDE)
    settle(t)


def test_sgm_average(pf):
    t = Tally("sgm_average")
    p1, p2, q1, q2, thr = PENALTIES[0]
    cases = [(kind, shape, ki) for ki, kind in enumerate(KINDS) for shape in SHAPES] + [("wide", SGM_WIDE, 9)]
    for kind, (H, W, D), ki in cases:
        L, R = wide_pair() if kind == "wide" else image_pair(kind, H, W)
        rng = np.random.default_rng(ki * 100 + D)
        vl, vr = volume(rng, D, H, W), volume(rng, D, H, W)
        a, b = vl.copy(), vr.copy()
        wl, wr = ref(pf.SGM_average, a, b, L, R, p1, p2, q1, q2, thr, SGM_V)
        c, d = vl.copy(), vr.copy()
        gl, gr = o.SGM_average(c, d, L, R, p1, p2, q1, q2, thr, SGM_V)
        what = "%s %dx%dx%d" % (kind, H, W, D)
        t.bits(gl, wl, what + " left")
        t.bits(gr, wr, what + " right")
        t.bits(c, a, what + " left input as the reference leaves it")
        t.bits(d, b, what + " right input as the reference leaves it")
    settle(t)


def test_sgm_nan_departure(pf):
    """The one stated departure.  One NaN at (d0, h0, w0), direction right: the reference's costs
    of row h0 are NaN at every disparity from w0 + 1 to the end of the row (np.amin of the previous pixel's costs is NaN,
    pf:551-566); the oracle's are finite there at every disparity but d0 (the NaN travels along its own plane as item1 and
    never enters the minimum over the line).  Rows without a NaN are the same bits on both sides."""
    t = Tally("nan")
    H, W, D = 4, 11, 6
    d0, h0, w0 = 2, 1, 3
    L, R = image_pair("smooth", H, W)
    vol = volume(np.random.default_rng(9), D, H, W)
    vol[d0, h0, w0] = np.nan
    p1, p2, q1, q2, thr = PENALTIES[0]
    for ch in "LR":
        want = ref(pf.semi_global_matching, L, R, vol.copy(), (0, 1), p1, p2, q1, q2, thr, ch)
        got = o.semi_global_matching(L, R, vol.copy(), (0, 1), p1, p2, q1, q2, thr, ch)
        assert np.isnan(want[:, h0, w0 + 1:]).all(), "the reference no longer propagates the NaN along the path"
        # pymin(NaN, x) is NaN like Python's min(nan, x), and `v < m` never takes a NaN: it stays on its own disparity
        assert np.isnan(got[d0, h0, w0:]).all(), "the oracle's NaN left its disparity plane"
        assert np.isfinite(np.delete(got[:, h0, w0:], d0, axis=0)).all(), "the oracle no longer drops the NaN"
        rows = [h for h in range(H) if h != h0]
        t.bits(got[:, rows], want[:, rows], "rows without a NaN " + ch)
        t.bits(got[:, h0, :w0], want[:, h0, :w0], "row h0 in front of the NaN " + ch)
    # A NaN on plane 0 is the exception: the oracle's minimum over the line starts from plane 0 and `v < m` never replaces
    # a NaN, so the minimum is NaN and every cost behind it is NaN - the reference's behaviour, all bits equal.
    vol = volume(np.random.default_rng(10), D, H, W)
    vol[0, h0, w0] = np.nan
    for ch in "LR":
        want = ref(pf.semi_global_matching, L, R, vol.copy(), (0, 1), p1, p2, q1, q2, thr, ch)
        got = o.semi_global_matching(L, R, vol.copy(), (0, 1), p1, p2, q1, q2, thr, ch)
        assert np.isnan(want[:, h0, w0 + 1:]).all() and np.isnan(got[:, h0, w0 + 1:]).all()
        t.bits(got, want, "NaN on plane 0 " + ch)
    settle(t)


# ---- a7 .. a11 ----------------------------------------------------------------------------------------------------------
def test_wta_to_bilateral(pf):
    t = Tally("post")
    shapes = SHAPES + ((5, 7, 1), (4, 1, 3))                 # one disparity plane; a single column
    for ki, kind in enumerate(KINDS):
        for H, W, D in shapes:
            img = image_pair(kind, H, W)[0]
            rng = np.random.default_rng(ki * 100 + H * W)
            vl, vr = (np.round(rng.uniform(0, 4, (D, H, W)) * 2) / 2 for _ in range(2))     # halves: ties
            vl, vr = vl.astype(np.float32), vr.astype(np.float32)
            what = "%s %dx%dx%d " % (kind, H, W, D)
            wdl, wdr = ref(pf.disparity_prediction, vl, vr)
            dl, dr = o.disparity_prediction(vl, vr)
            t.bits(dl, wdl, what + "wta left")
            t.bits(dr, wdr, what + "wta right")
            wi = ref(pf.interpolation, wdl, wdr, D)
            t.bits(o.interpolation(wdl, wdr, D), wi, what + "interpolation")
            ws = ref(pf.subpixel_enhance, wi, vl)
            t.bits(o.subpixel_enhance(wi, vl), ws, what + "sub-pixel")
            for fh, fw in WINDOWS:
                wm = ref(pf.median_filter, ws, fh, fw)
                t.bits(o.median_filter(ws, fh, fw), wm, what + "median %dx%d" % (fh, fw))
                for sigma, thr in BILATERAL:
                    wb = ref(pf.bilateral_filter, img, wm, fh, fw, 0, sigma, thr)
                    t.bits(o.bilateral_filter(img, wm, fh, fw, 0, sigma, thr), wb,
                           what + "bilateral %dx%d sigma %g threshold %g" % (fh, fw, sigma, thr))
    settle(t)


# ---- a2 -----------------------------------------------------------------------------------------------------------------
def test_cost_volume(pf):
    t = Tally("cost_volume")
    for H, W, D, C in CV_SHAPES:
        rng = np.random.default_rng(H * W + D)
        fl, fr = (rng.standard_normal((H, W, C)).astype(np.float32) for _ in range(2))
        for special in (False, True):
            if special:
                fl, fr = fl.copy(), fr.copy()
                fl[H // 2, W // 3, C // 2] = np.nan
                fr[0, W - 2, 1] = np.inf
            what = "%dx%dx%d C=%d%s" % (H, W, D, C, " with NaN and inf" if special else "")
            wl, wr = ref(pf.compute_cost_volume, fl, fr, D)
            with np.errstate(all="ignore"):
                gl, gr = o.compute_cost_volume(fl, fr, D)
            t.bits(gl, wl, what + " left")
            t.bits(gr, wr, what + " right")
    settle(t)


# ---- outside the reference's domain -------------------------------------------------------------------------------------
def test_inputs_the_reference_refuses(pf):
    """REFUSED, in order: the reference raises what is listed there (anything else fails the test), nothing is compared,
    and the oracle takes the input."""
    t = Tally("refused")
    raised = []
    img = image_pair("smooth", 5, 8)[0]
    vol = volume(np.random.default_rng(3), 1, 5, 8)
    nan_column = volume(np.random.default_rng(4), 3, 5, 8)
    nan_column[:, 2, 5] = np.nan
    calls = ((lambda: ref(pf.compute_cross_region, img, 0, 14), lambda: o.cross_arms(img, 0, 14)),
             (lambda: ref(pf.semi_global_matching, img, img, vol.copy(), (0, 1), 2.3, 55.9, 4, 8, 0.08, "L"),
              lambda: o.semi_global_matching(img, img, vol.copy(), (0, 1), 2.3, 55.9, 4, 8, 0.08, "L")),
             (lambda: ref(pf.disparity_prediction, nan_column, nan_column),
              lambda: o.disparity_prediction(nan_column, nan_column)))
    assert len(calls) == len(REFUSED)
    for (what, exc), (reference_call, oracle_call) in zip(REFUSED, calls):
        with pytest.raises(exc):
            reference_call()
        raised.append(what)
        oracle_call()
        t.total += 1
    print("the reference raised for: %s" % "; ".join(raised))
    settle(t)
