"""No GPU: the restatements of tests/paper_rules_reference.py pinned against each other and against the oracle, so that
test_paper_rules_gpu.py compares the kernels with something already checked.

  both_views_iter   == the literal triple loop (cbca_both_check); == the oracle's aggregation where the intersection
                    changes nothing (identical views at d = 0, planes without a partner); == a float64 sum rounded once on
                    integer volumes (written through row prefix sums: no code shared with the step loop)
  interpolate_ex    (4, right) == post_reference.interpolate; == the literal of test_extras_gpu.py; the shared case set
                    reaches every neighbour count
  subpixel_numpy1   == the literal of test_extras_gpu.py; != the float32 chain on the case set, == it where nothing is fitted
  match_paper       with every extra off == paper_sgm_reference.match_from_cost_volumes"""
import numpy as np
import pytest

import oracle as o
import paper_rules_reference as pr
import paper_sgm_reference as psr
import post_reference as ref
from helpers import Tally, assert_bits


def _blocks(H, W, key):
    """Piecewise-constant views with a few levels: arms of every length, ragged regions."""
    rng = pr.case_rng(50, H, W, key)
    a = rng.integers(0, 3, size=(H // 3 + 1, W // 4 + 1)).astype(np.float32)
    img = np.kron(a, np.ones((3, 4), dtype=np.float32))[:H, :W]
    other = np.roll(img, 2, axis=1) + (rng.random((H, W)) < 0.1).astype(np.float32)
    return np.ascontiguousarray(img), np.ascontiguousarray(other.astype(np.float32))


SMALL = [(5, 9, 4), (7, 12, 3), (6, 11, 13), (1, 8, 3), (9, 1, 2)]      # (H, W, D); D = 13 > W: planes without partner


@pytest.mark.parametrize("L", [1, 2, 14, 15, 32])
def test_both_views_iter_equals_the_literal_triple_loop(L):
    t = Tally("both_views_iter against cbca_both_check, L=%d" % L)
    for si, (H, W, D) in enumerate(SMALL):
        for kind in ("constant", "blocks"):
            a, b = (np.full((H, W), 0.5, np.float32),) * 2 if kind == "constant" else _blocks(H, W, si)
            arms_a, arms_b = o.cross_arms(a, pr.CBCA_TAU, L)[0], o.cross_arms(b, pr.CBCA_TAU, L)[0]
            if kind == "constant":
                assert int(arms_a.max()) == min(L, max(H, W)) - 1
            for vk in ("random", "special"):
                vol = pr.volume(vk, D, H, W, si)
                for side, own, other in ((0, arms_a, arms_b), (1, arms_b, arms_a)):
                    got = pr.both_views_iter(vol, own, other, side, pr.clamp_of(L))
                    t.bits(got, pr.cbca_both_check(vol, own, other, side), "%s %s %s side %d" % ((H, W, D), kind, vk, side))
    t.settle(floor=len(SMALL) * 2 * 2 * 2)


def test_both_views_iter_clamps_own_arms_only():
    """R below the own arms: the literal loop on own arms clamped beforehand (the partner's are not clamped - the minimum
    with a clamped arm cannot exceed R anyway)."""
    H, W, D = 8, 21, 5
    a = np.full((H, W), 0.5, np.float32)
    arms = o.cross_arms(a, pr.CBCA_TAU, 32)[0]
    assert int(arms.max()) == 20
    vol = pr.volume("random", D, H, W, 3)
    for side in (0, 1):
        assert_bits(pr.both_views_iter(vol, arms, arms, side, 13), pr.cbca_both_check(vol, np.minimum(arms, 13), arms, side),
                    "clamp to 13, side %d" % side)


@pytest.mark.parametrize("L", [2, 14, 32])
def test_both_views_iter_equals_the_oracle_where_the_intersection_changes_nothing(L):
    H, W = 12, 19
    D = W + 2
    img, other = _blocks(H, W, L)
    arms, arms_other = o.cross_arms(img, pr.CBCA_TAU, L)[0], o.cross_arms(other, pr.CBCA_TAU, L)[0]
    vol = pr.volume("special", D, H, W, L)
    want = o.cost_volume_aggregation(img, img, vol, vol, pr.CBCA_TAU, L, 1)[0]
    R = pr.clamp_of(L)
    # identical views: at d = 0 every pixel is its own partner
    for side in (0, 1):
        assert_bits(pr.both_views_iter(vol[:1], arms, arms, side, R), want[:1], "identical views, d = 0, side %d" % side)
    # d >= W: no pixel has a partner, whatever the other view holds
    for side in (0, 1):
        got = pr.both_views_iter(vol, arms, arms_other, side, R)
        assert_bits(got[W:], want[W:], "planes d >= W, side %d" % side)
        assert not np.array_equal(got[1], want[1], equal_nan=True)          # and the intersection does change the others


def _float64_region_mean(vol, eff):
    """sum over the region in float64 through row prefix sums, / count, rounded to float32 once."""
    D, H, W = vol.shape
    xs = np.arange(W)
    c = np.concatenate([np.zeros((D, H, 1)), np.cumsum(vol.astype(np.float64), axis=2)], axis=2)
    lo, hi = xs - eff[..., 2], xs + eff[..., 3] + 1
    rows = np.take_along_axis(c, hi, axis=2) - np.take_along_axis(c, lo, axis=2)          # [D,H,W]: row q's arm at x
    cnt = (eff[..., 2] + eff[..., 3] + 1).astype(np.float64)
    out = np.empty((D, H, W), dtype=np.float32)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                u, dn = eff[d, y, x, 0], eff[d, y, x, 1]
                out[d, y, x] = np.float32(rows[d, y - u:y + dn + 1, x].sum() / cnt[d, y - u:y + dn + 1, x].sum())
    return out


@pytest.mark.parametrize("L", [14, 32])
def test_both_views_iter_on_integers_is_the_float64_mean_rounded_once(L):
    """|c| <= 1023 and at most 63 x 63 elements: every partial sum is an integer below 2^24, so float32 adds are exact and
    their order cannot matter; float32(s) / float32(n) is the correctly rounded quotient, and so is the float64 quotient
    rounded to float32 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous)."""
    H, W, D = 14, 33, 6
    for kind in ("constant", "blocks"):
        a, b = (np.full((H, W), 0.5, np.float32),) * 2 if kind == "constant" else _blocks(H, W, 7)
        arms_a, arms_b = o.cross_arms(a, pr.CBCA_TAU, L)[0], o.cross_arms(b, pr.CBCA_TAU, L)[0]
        vol = pr.volume("integer", D, H, W, 1)
        assert np.abs(vol).max() <= 1023 and np.array_equal(vol, np.round(vol))
        for side, own, other in ((0, arms_a, arms_b), (1, arms_b, arms_a)):
            R = pr.clamp_of(L)
            eff = pr.both_view_arms(own, other, side, D, R)
            assert_bits(pr.both_views_iter(vol, own, other, side, R), _float64_region_mean(vol, eff),
                        "integer volume %s side %d" % (kind, side))


def _against_the_literals(t, what, dl, st):
    t.bits(pr.interpolate_ex(dl, st, 4, False), ref.interpolate(dl, st), what + " post_reference")
    for directions, occ in pr.INTERP_MODES:
        t.bits(pr.interpolate_ex(dl, st, directions, occ), pr.interpolate_check(dl, st, directions, occ),
               what + " literal (%d, %s)" % (directions, occ))


# the literals index NumPy arrays pixel by pixel: the shapes of the shared set they walk in a second or two, and two
# ragged ones of their own
LITERAL_SHAPES = [si for si, (H, W) in enumerate(pr.INTERP_SHAPES) if H * W <= 64]


@pytest.mark.parametrize("si", LITERAL_SHAPES, ids=["%dx%d" % pr.INTERP_SHAPES[si] for si in LITERAL_SHAPES])
def test_interpolate_ex_equals_the_other_statements(si):
    """(4, right) is the reference's rule: post_reference.interpolate, on every status map (both leave a pixel whose
    word is none of 0 / 1 / 2 as it is); all four modes equal test_extras_gpu.py's literal where that one is quick."""
    t = Tally("interpolate_ex %dx%d" % pr.INTERP_SHAPES[si])
    for sk, mk, dl, st in pr.interpolation_cases(si):
        _against_the_literals(t, "%s %s" % (sk, mk), dl, st)
    t.settle(floor=len(pr.STATUS_KINDS) * len(pr.MAP_KINDS) * 5)


@pytest.mark.parametrize("shape", [(9, 14), (5, 40)], ids=["9x14", "5x40"])
def test_interpolate_ex_equals_the_other_statements_on_ragged_maps(shape):
    t = Tally("interpolate_ex %dx%d" % shape)
    for ki, sk in enumerate(pr.STATUS_KINDS):
        for mi, mk in enumerate(pr.MAP_KINDS):
            rng = pr.case_rng(31, shape[0], ki, mi)
            _against_the_literals(t, "%s %s" % (sk, mk), pr.disparity_map(mk, shape[0], shape[1], rng),
                                  pr.status_map(sk, shape[0], shape[1], rng))
    t.settle(floor=len(pr.STATUS_KINDS) * len(pr.MAP_KINDS) * 5)


def test_interpolation_cases_reach_every_neighbour_count():
    seen = {4: set(), 16: set()}
    odd = nan_neighbour = 0
    for si in range(len(pr.INTERP_SHAPES)):
        for sk, mk, dl, st in pr.interpolation_cases(si):
            for directions in (4, 16):
                out, counts = pr.interpolate_ex(dl, st, directions, False, return_counts=True)
                seen[directions] |= set(np.unique(counts[counts >= 0]).tolist())
                nan_neighbour += int((np.isnan(out) & (st == 1) & ~np.isnan(dl)).sum())
            odd += int((~np.isin(st, (0, 1, 2))).sum())
    assert seen[16] == set(range(17)), sorted(seen[16])
    assert seen[4] == set(range(5)), sorted(seen[4])
    assert odd > 100 and nan_neighbour > 100            # words other than 0 / 1 / 2; medians that a NaN neighbour decides


def test_median_with_a_nan_neighbour_is_nan():
    """The rule the kernels' median follows since this file exists: np.median, wherever the NaN stands."""
    dl = np.array([[np.nan, 5, 1, 7, 2]], dtype=np.float32)
    st = np.array([[0, 1, 0, 1, 0]], dtype=np.int32)
    out = pr.interpolate_ex(dl, st, 4, False)
    assert np.isnan(out[0, 1]) and out[0, 3] == 1.5


@pytest.mark.parametrize("D", pr.SUBPIXEL_D)
def test_subpixel_numpy1_against_the_float32_chain(D):
    differs = 0
    for kind in pr.CURVE_KINDS:
        d, vol = pr.subpixel_case(D, kind)
        got = pr.subpixel_numpy1(d, vol)
        plain = ref.subpixel_enhance(d, vol)
        edge = ((d - np.float32(1)).astype(np.int64) < 0) | ((d + np.float32(1)).astype(np.int64) >= D)
        assert edge.any()
        assert_bits(got[edge], plain[edge], "D=%d %s: nothing fitted at the ends" % (D, kind))
        assert_bits(got[edge], d[edge], "D=%d %s: the raw value" % (D, kind))
        differs += int((got.view(np.uint32) != plain.view(np.uint32)).sum())
        with np.errstate(all="ignore"):          # the literal of test_extras_gpu.py: the same float32 index expressions
            assert_bits(got, pr.numpy1_subpixel_check(d, vol), "D=%d %s: literal" % (D, kind))
        if kind == "huge" and D >= 12:
            # 2 C overflows in float32: the denominator is +-inf there, the quotient 0 and the float32 chain returns d;
            # the float64 denominator is finite
            flushed = ~edge & (plain == d) & (got != d)
            assert flushed.any()
    assert differs > 0 or D == 2


def test_match_paper_with_every_extra_off_is_the_plain_chain():
    H, W, D = 20, 36, 6
    import synthetic
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=12)
    rng = pr.case_rng(60)
    f = rng.standard_normal((2, H, W, 64)).astype(np.float32)
    f /= np.linalg.norm(f, axis=-1, keepdims=True)
    cv = o.compute_cost_volume(f[0], np.roll(f[0], -2, axis=1) + 0.1 * f[1], D)
    hp = dict(cbca_num_iterations2=3)
    for independent in (False, True):
        want, stages = psr.match_from_cost_volumes(L, R, cv[0], cv[1], D, independent, hp, return_all=True)
        got, mine = pr.match_paper(L, R, cv[0], cv[1], D, dict(sgm_independent_directions=independent), hp)
        assert_bits(got, want, "final map")
        for k, v in stages.items():
            for a, b in zip(mine[k] if isinstance(v, tuple) else (mine[k],), v if isinstance(v, tuple) else (v,)):
                assert_bits(a, b, k)
