"""CPU: the oracle's post-processing stages (oracle/mccnn_oracle.c, a7-a11) pinned to the literal NumPy reference of
tests/post_reference.py at the edges the golden pairs never reach: images smaller than the window, windows from 1x1 to
the 49-tap limit, ties, NaN / +-inf / +-0 / -1 in the maps, a NaN image pixel, left-right maps with fractional, out of
range and non-finite values.  Every comparison is on uint32 patterns (helpers.bits_strict: signs of zeros count, NaN
payloads do not) and excludes no pixel and no case.  Once this holds, the GPU tests may use the oracle as their fast
witness (test_post_edges_gpu.py does, for the shapes the literal's Python loops are too slow for).

What it found when written: np.median ends in np.mean, whose float32 sum starts from +0, so a median of -0.0 is +0.0;
orc_median and median_small returned -0.0 (45 of the 468 median cases and 4 interpolation pixels in 2 of 30 cases
differed, every one only in the sign of a zero; nothing else differed).  The oracle's left-right check also indexed the
right map out of bounds for a left disparity of -1 or NaN (mccnn_wta's "no winner"), where include/mccnn.h says
"occlusion": it has the header's guard now, for values <= -1 and NaN only - a value in (-1, 0) truncates to 0 in the
reference, where the kernels used to say "occlusion"."""
import numpy as np
import pytest

import post_reference as ref
from helpers import _describe, bits_strict


def settle(failures, total, what):
    assert not failures, "%s: %d of %d cases differ from the literal reference:\n%s" % (
        what, len(failures), total, "\n".join(failures[:40]))


@pytest.mark.parametrize("wi", range(len(ref.WINDOWS)), ids=["%dx%d" % w for w in ref.WINDOWS])
def test_median_oracle_against_literal(wi):
    import oracle as o
    fh, fw = ref.WINDOWS[wi]
    failures, total = [], 0
    for shape, kind, m in ref.median_cases(wi):
        total += 1
        got, want = o.median_filter(m, fh, fw), ref.median_filter(m, fh, fw)
        if not bits_strict(got, want):
            failures.append("median %dx%d on %s %s: %s" % (fh, fw, shape, kind, _describe(got, want)))
    settle(failures, total, "median %dx%d" % (fh, fw))


def test_median_of_negative_zero_is_positive_zero():
    """np.mean's float32 sum starts from +0: one value -0.0, or two middle values -0.0, give +0.0."""
    import oracle as o
    nz = np.float32(-0.0)
    for m, win in ((np.array([[nz]]), (1, 1)), (np.array([[nz]]), (5, 5)), (np.array([[nz, nz]]), (1, 3)),
                   (np.array([[-1, nz, 2]], dtype=np.float32), (1, 3)),
                   (np.array([[-1, nz], [nz, 3]], dtype=np.float32), (3, 3))):
        m = m.astype(np.float32)
        want = ref.median_filter(m, *win)
        assert not np.signbit(want).all()                      # NumPy does turn some of them
        got = o.median_filter(m, *win)
        assert bits_strict(got, want), "%s %s: %s" % (m.tolist(), win, _describe(got, want))


@pytest.mark.parametrize("wi", range(len(ref.WINDOWS)), ids=["%dx%d" % w for w in ref.WINDOWS])
def test_bilateral_oracle_against_literal(wi):
    import oracle as o
    fh, fw = ref.WINDOWS[wi]
    failures, total = [], 0
    for shape, kind, img, m in ref.bilateral_cases(wi):
        for sigma, thr in ref.BILATERAL_SETTINGS:
            total += 1
            got = o.bilateral_filter(img, m, fh, fw, 0, sigma, thr)
            want = ref.bilateral_filter(img, m, fh, fw, 0, sigma, thr)
            if not bits_strict(got, want):
                failures.append("bilateral %dx%d sigma %g thr %g on %s %s: %s"
                                % (fh, fw, sigma, thr, shape, kind, _describe(got, want)))
    settle(failures, total, "bilateral %dx%d" % (fh, fw))


def test_bilateral_gated_out_taps_still_count():
    """NumPy multiplies a shut gate (0) with the tap's disparity: 0 * NaN = NaN, 0 * inf = NaN.  A threshold of 0 shuts
    every gate, the centre's included: 0 / 0 everywhere."""
    import oracle as o
    img = np.zeros((5, 6), dtype=np.float32)
    img[2, 3] = 10                                     # gated out of every neighbour's window (threshold 2)
    for bad in (np.nan, np.inf, -np.inf):
        m = np.ones((5, 6), dtype=np.float32)
        m[2, 3] = bad
        want = ref.bilateral_filter(img, m, 3, 3, 0, 6, 2)
        assert np.isnan(want[1:4, 2:5]).sum() >= 8 and np.isfinite(want[0, 0])
        assert bits_strict(o.bilateral_filter(img, m, 3, 3, 0, 6, 2), want)
    m = np.arange(30, dtype=np.float32).reshape(5, 6)
    want = ref.bilateral_filter(img, m, 5, 5, 0, 6, 0)
    assert np.isnan(want).all()
    assert bits_strict(o.bilateral_filter(img, m, 5, 5, 0, 6, 0), want)


def test_lr_status_oracle_against_literal():
    import oracle as o
    failures, total, seen = [], 0, set()
    for shape, match, special, dl, dr in ref.lr_cases():
        total += 1
        D = shape[2]
        got, want = o.lr_status(dl, dr, D), ref.lr_status(dl, dr, D)
        seen |= set(np.unique(want).tolist())
        # the header's contract where the reference is undefined: asserted, not excluded
        undefined = ~(dl > -1)
        assert (got[undefined] == 2).all() and (want[undefined] == 2).all()
        if not np.array_equal(got, want):
            failures.append("lr_status %s match %g special %s: %d differ" % (shape, match, special, (got != want).sum()))
    assert seen == {0, 1, 2}
    settle(failures, total, "lr_status")


def test_interpolation_oracle_against_literal():
    import oracle as o
    failures, total, seen = [], 0, set()
    for shape, match, special, dl, dr in ref.lr_cases():
        total += 1
        D = shape[2]
        st = ref.lr_status(dl, dr, D)
        seen |= set(np.unique(st).tolist())
        got, want = o.interpolation(dl, dr, D), ref.interpolation(dl, dr, D)
        if not bits_strict(got, want):
            failures.append("interpolation %s match %g special %s: %s" % (shape, match, special, _describe(got, want)))
    assert seen == {0, 1, 2}
    settle(failures, total, "interpolation")


def test_subpixel_oracle_against_literal():
    import oracle as o
    failures, total, changed = [], 0, 0
    for shape, d, vol in ref.subpixel_cases():
        total += 1
        got, want = o.subpixel_enhance(d, vol), ref.subpixel_enhance(d, vol)
        changed += int((want != d).sum())
        keep = d == -1
        assert bits_strict(want[keep], d[keep])              # "no winner" passes through
        if not bits_strict(got, want):
            failures.append("subpixel %s: %s" % (shape, _describe(got, want)))
    assert changed > 50
    settle(failures, total, "subpixel")


def test_disparity_prediction_oracle_against_literal():
    import oracle as o
    total, none = 0, 0
    for vol in ref.wta_volumes():
        total += 1
        got, want = o.disparity_prediction(vol, vol[:, ::-1].copy()), ref.disparity_prediction(vol, vol[:, ::-1].copy())
        none += int((want[0] == -1).sum())
        for g, w in zip(got, want):
            assert bits_strict(g, w), "WTA %s: %s" % (vol.shape, _describe(g, w))
    assert none >= 2 * (total - 6)                                     # the all-NaN and all-+inf pixels give -1
