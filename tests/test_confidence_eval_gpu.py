"""GPU: evaluation.sparsification (torch on the device) against the restatement of tests/confidence_reference.py on maps
with ties, NaN confidences, invalid estimates, pixels outside the region and an empty region.  n and e are integers and
must be exact.  Both sides add n float64 terms in [0, 1], each the same correctly rounded quotient, and divide by n: a sum
of n such terms is off by less than n * (n * 2^-53) whatever the order, the quotient by n * 2^-53, so the two figures
differ by at most n * 2^-52 - the bound asserted here."""
import numpy as np
import pytest
import torch

import confidence_reference as ref

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(H, W, seed, ties, empty=False):
    rng = np.random.default_rng(seed)
    gt = (rng.random((H, W)) * 20).astype(np.float32)
    gt[rng.random((H, W)) < 0.15] = np.inf                                    # outside the region
    disp = (gt + rng.standard_normal((H, W)) * 1.2).astype(np.float32)
    disp[~np.isfinite(disp)] = 3.0
    for val in (-1.0, np.nan, np.inf, -0.0):                                   # invalid estimates, and a valid -0.0
        disp[rng.random((H, W)) < 0.03] = np.float32(val)
    if empty:
        gt[:] = np.inf
    conf = rng.standard_normal((4, H, W)).astype(np.float32)
    if ties:
        conf = np.round(conf * 2) / 2                                         # nine levels: long runs of equal keys
        conf[conf == 0] = np.where(rng.random(int((conf == 0).sum())) < 0.5, 0.0, -0.0)
    conf[3] = -np.abs(np.round(conf[3]))
    for val in (np.nan, -np.inf, np.inf):
        conf[rng.random((4, H, W)) < 0.04] = np.float32(val)
    return disp, gt, conf.astype(np.float32)


def restated_bad(disp, gt, T):
    region = np.isfinite(gt)
    invalid = ~np.isfinite(disp) | (disp < 0)
    with np.errstate(invalid="ignore"):
        err = np.abs(disp - np.where(region, gt, np.float32(0)))
        return (invalid | (err > np.float32(T))) & region, region


@pytest.mark.parametrize("H,W,ties,empty", [(1, 1, False, False), (7, 9, True, False), (40, 48, False, False),
                                            (40, 48, True, False), (61, 97, True, False), (12, 20, True, True)])
def test_sparsification_against_the_restatement(H, W, ties, empty):
    import evaluation as ev
    disp, gt, conf = make_case(H, W, H * W, ties, empty)
    bad, region = ev.bad_and_region(dev(disp), dev(gt), 1.0)
    want_bad, want_region = restated_bad(disp, gt, 1.0)
    assert np.array_equal(bad.cpu().numpy(), want_bad) and np.array_equal(region.cpu().numpy(), want_region)
    got = ev.sparsification(dev(conf), bad, region)
    assert got.dtype == torch.float64 and tuple(got.shape) == (7,) and got.is_cuda
    got = got.cpu().numpy()
    for i, name in enumerate(ref.NAMES):
        want = ref.sparsification(conf[i], want_bad, want_region)
        n, e = want["n"], want["e"]
        print("%dx%d %s: n %d e %d auc %.17g (restated %.17g) optimal %.17g (restated %.17g)" % (
            W, H, name, n, e, got[3 + i], want["auc"], got[2], want["auc_optimal"]))
        assert got[0] == n and got[1] == e
        if n == 0:
            assert empty and np.isnan(got[2]) and np.isnan(got[3 + i])
            continue
        assert abs(got[3 + i] - want["auc"]) <= n * 2.0 ** -52
        assert abs(got[2] - want["auc_optimal"]) <= n * 2.0 ** -52
    figures = ev.sparsification_figures(got, ref.NAMES, 1.0)
    assert sorted(figures) == ["auc", "auc_optimal", "bad_rate", "n", "threshold"] and sorted(figures["auc"]) == sorted(ref.NAMES)
    assert figures["n"] == want["n"] and figures["bad_rate"] == (want["e"] / want["n"] if want["n"] else None)


def test_nothing_blocks_the_host():
    """The score is enqueued behind a pair on the pair's stream: no step of it may make the host wait for the device (a
    device tensor built from a host scalar, an .item(), a data-dependent shape).  torch reports every such
    synchronisation as an error in this mode.  Both rules, through Sparsifier.score as match.py calls it."""
    import evaluation as ev
    disp, gt, conf = make_case(40, 48, 7, True)
    code = np.where(np.isfinite(gt), np.clip(np.rint(gt * 256), 1, 65535), 0).astype(np.uint16)
    d, g, c, k = dev(disp), dev(gt), dev(conf), dev(code)
    mb, kitti = ev.Sparsifier(ref.NAMES, 1.0), ev.Sparsifier(ref.NAMES, (3.0, 0.05))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bad, region = ev.bad_and_region(d, g, 1.0)
        ev.sparsification(c, bad, region)
        scores = [mb.score(d, c, g), kitti.score(d, c, k)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    figures = [s.figures() for s in scores]
    want_bad, want_region = restated_bad(disp, gt, 1.0)
    want = ref.sparsification(conf[0], want_bad, want_region)
    assert figures[0]["n"] == want["n"] and abs(figures[0]["auc"]["msm"] - want["auc"]) <= want["n"] * 2.0 ** -52
    assert figures[1]["n"] == int((code != 0).sum()) and figures[1]["threshold"] == [3.0, 0.05]


def test_kitti_rule():
    """bad_and_region_kitti: region gt_occ != 0; bad = invalid, or err above abs AND above rel * truth, in float32."""
    import evaluation as ev
    rng = np.random.default_rng(3)
    H, W = 30, 44
    code = rng.integers(0, 120 * 256, (H, W)).astype(np.uint16)
    code[rng.random((H, W)) < 0.3] = 0
    g = code.astype(np.float32) / np.float32(256)
    disp = (g + rng.standard_normal((H, W)) * 3).astype(np.float32)
    disp[rng.random((H, W)) < 0.05] = np.nan
    bad, region = ev.bad_and_region_kitti(dev(disp), dev(code.astype(np.int32)), 3.0, 0.05)
    with np.errstate(invalid="ignore"):
        err = np.abs(disp - g)
        want = (~np.isfinite(disp) | (disp < 0) | ((err > np.float32(3)) & (err > np.float32(0.05) * g))) & (code != 0)
    assert np.array_equal(region.cpu().numpy(), code != 0) and np.array_equal(bad.cpu().numpy(), want)
    assert want.any() and (~want & (code != 0)).any()
