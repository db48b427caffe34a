"""CPU: what tests/test_accurate_edges_gpu.py stands on.  The voxel sample of its large shapes holds every seam of the
decision kernel's tiling and stays small; on its inputs a voxel that was written to a neighbour's place is ten times
beyond the bound it is compared under; the two helpers that restate the kernel from its own inputs and the borders
column by column agree with the restatements the rest of the suite uses."""
import functools

import numpy as np
import pytest
import torch

import accurate_reference as ar
import helpers
import tolerances as tol

NAMES = list(ar.EDGE_CASES)


def _net(C, n_fc, patch, seed=11):
    from model import ACCURATE_NET
    return ACCURATE_NET(None, input_patch_size=patch, num_conv_layers=(patch - 1) // 2, num_conv_feature_maps=C,
                        num_fc_layers=n_fc, batch_size=1, device="cpu", seed=seed)      # seeded glorot


@functools.lru_cache(maxsize=None)
def _case(name):
    """The network of the GPU test (same seed), the tower outputs of its smooth pair by the float64 restatement
    (rounded to float32, as the GPU hands them on) and the sample."""
    H, W, D, C, n_fc, patch = ar.EDGE_CASES[name]
    conv, fc = ar.net_lists(_net(C, n_fc, patch))
    L, R = helpers.smooth_pair(H, W, seed=H + W)
    fl, fr = (ar.image_features_float64(conv, t).float() for t in (L, R))
    return dict(H=H, W=W, D=D, fc=fc, fl=fl, fr=fr, sample=ar.edge_sample(name))


@pytest.mark.parametrize("name", NAMES)
def test_sample_holds_every_seam_and_only_valid_voxels(name):
    c = _case(name)
    H, W, D = c["H"], c["W"], c["D"]
    h, w, d = c["sample"]
    assert h.dtype == w.dtype == d.dtype == np.int64 and h.shape == w.shape == d.shape
    assert (0 <= h).all() and (h < H).all() and (0 <= d).all() and (d < D).all() and (w < W).all()
    assert (w >= d).all(), "an invalid voxel (w < d) was sampled"
    assert len(h) <= ar.EDGE_SAMPLE_CAP
    have = set(zip(h.tolist(), w.tolist(), d.tolist()))
    # the seams, spelled out here independently of seam_voxels()
    missing = []
    for dd in range(D):
        if dd % 32 not in (0, 31) and dd != D - 1:
            continue
        ws = [dd, dd + 1, dd + 3, dd + 4, W - 2, W - 1]
        ws.append(next(x for x in range(dd, dd + 4) if x % 4 == 0))
        ws.append(next(x for x in range(dd, dd + 4) if x % 4 == 3))
        for ww in ws:
            if ww >= W:                                      # d + 3, d + 4 next to the last disparities: no such pixel
                continue
            for hh in range(H):
                if (hh, ww, dd) not in have:
                    missing.append((hh, ww, dd))
    assert not missing, "%d seam voxels are not in the sample, e.g. %s" % (len(missing), missing[:5])
    n_seams = len(ar.seam_voxels(H, W, D))
    assert len(h) == n_seams + ar.EDGE_RANDOM_VOXELS
    # the random part is spread over the disparity blocks: every full 32-block of d is hit
    assert set((d[n_seams:] // 32).tolist()) >= set(range(D // 32))
    # and the draw is repeatable
    again = ar.edge_sample(name)
    assert all(np.array_equal(a, b) for a, b in zip(c["sample"], again))


@pytest.mark.parametrize("name", NAMES)
def test_a_misplaced_voxel_is_ten_bounds_away(name):
    """At least 99 % of the sampled voxels differ from their neighbour in d and from their neighbour in w by at least
    10 x the bound the GPU test applies (ACCURATE_SPLIT_E32_FACTOR x E32 of the same sample).  Neighbour in d: d + 1,
    on the diagonal (w = d, where d + 1 is no voxel) d - 1; the voxels (h, 0, 0) have neither and count as not
    distinguishable.  Neighbour in w: w - 1, on the diagonal w + 1."""
    c = _case(name)
    h, w, d = c["sample"]
    s64, e32, e16 = ar.sampled_yardsticks(c["fc"], c["fl"], c["fr"], c["sample"])
    bound = tol.ACCURATE_SPLIT_E32_FACTOR * e32
    assert 0.0 < e32 < e16 and bound < 1e-6
    dn = np.where(d + 1 <= w, d + 1, d - 1)
    has_dn = dn >= 0
    sd = ar.sampled_scores(c["fc"], c["fl"], c["fr"], (h[has_dn], w[has_dn], dn[has_dn]))
    diff_d = np.zeros(len(h))
    diff_d[has_dn] = np.abs(sd - s64[has_dn])
    wn = np.where(w - 1 >= d, w - 1, w + 1)
    assert (wn < c["W"]).all()
    diff_w = np.abs(ar.sampled_scores(c["fc"], c["fl"], c["fr"], (h, wn, d)) - s64)
    for what, diff in (("d", diff_d), ("w", diff_w)):
        frac = float((diff >= 10 * bound).mean())
        print("%s: neighbour in %s: E32 %.2e, bound %.2e, 1st percentile %.2e (%.0f x bound), 10th %.2e, %.4f beyond "
              "10 x bound" % (name, what, e32, bound, np.percentile(diff, 1), np.percentile(diff, 1) / bound,
                              np.percentile(diff, 10), frac))
        assert frac >= 0.99, "neighbours in %s: only %.4f of the sample is 10 bounds away" % (what, frac)


def test_decision_from_halves_is_the_decision_network():
    """From finite halves it is decision() on the concatenation (the first layer is linear in it), in every precision
    the yardsticks use; from poisoned halves it is IEEE arithmetic: NaN in, NaN out; -inf is relu's 0."""
    net = _net(64, 4, 9, seed=2)
    _conv, fc = ar.net_lists(net)
    g = torch.Generator().manual_seed(4)
    fl, fr = torch.rand((50, 64), generator=g), torch.rand((50, 64), generator=g)
    w1, b1 = fc[0][0].double(), fc[0][1].double()
    aL = fl.double() @ w1[:, :64].t() + b1
    aR = fr.double() @ w1[:, 64:].t()
    want = ar.decision(fc, torch.cat((fl, fr), -1))
    got = ar.decision_from_halves(fc, aL, aR)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-14
    got32 = ar.decision_from_halves(fc, aL.float(), aR.float(), torch.float32)
    assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) <= 1e-6
    got16 = ar.decision_from_halves(fc, aL, aR, torch.float64, True)
    assert 1e-7 < float((got16 - want).abs().max()) <= 1e-3          # f16 inputs: visibly rounded, still the network
    u0 = 5
    fcz = [(w.clone(), b.clone()) for w, b in fc]
    fcz[1][0][:, u0] = 0.0                                            # the unit reaches nothing downstream
    aL[:, u0] = 0.0
    aR[:, u0] = 0.0
    clean = ar.decision_from_halves(fcz, aL, aR)
    for value, poisoned in ((float("nan"), True), (float("inf"), True), (float("-inf"), False), (255.875, False)):
        bad = aL.clone()
        bad[7, u0] = value
        out = ar.decision_from_halves(fcz, bad, aR)
        assert bool(torch.isnan(out[7])) == poisoned, value           # (inf * the zero weight is NaN too)
        keep = torch.ones(50, dtype=torch.bool)
        keep[7] = poisoned is False
        assert torch.equal(out[keep], clean[keep]), value


def test_borders_by_column_are_the_literal_borders():
    """volumes_from_scores_by_column == volumes_from_scores bit for bit, NaN and inf scores included."""
    rng = np.random.default_rng(8)
    for D, H, W in ((2, 3, 4), (5, 2, 7), (33, 2, 36), (40, 1, 71)):
        s = -rng.random((D, H, W)).astype(np.float32)
        s[D - 1, 0, W - 1] = np.nan
        s[0, H - 1, 1] = -np.inf
        want = ar.volumes_from_scores(s.copy())
        got = ar.volumes_from_scores_by_column(s.copy())
        helpers.assert_bits_strict(got[0], want[0], "left volume %s" % ((D, H, W),))
        helpers.assert_bits_strict(got[1], want[1], "right volume %s" % ((D, H, W),))
