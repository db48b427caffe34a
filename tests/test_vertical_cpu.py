"""CPU: the cost volume's vertical search (include/mccnn.h: mccnn_cost_volume_vertical_hwd) - its NumPy restatement
tied to the pinned oracle at range 0, the entry point's validation, the flag / extra / switch, and the reason for it:
on pairs whose right image sits two rows low the plain matcher collapses and a vertical range of 2 recovers the map."""
import ctypes

import numpy as np
import pytest

from helpers import assert_bits
import paper_sgm_reference as ps
import vertical_reference as vr


# ---- the restatement at range 0 is the oracle ------------------------------------------------------------------------
def test_restatement_at_range_0_equals_the_oracle_on_the_golden_features(golden_cases):
    import oracle as o
    for name, g in golden_cases:
        D = g["cv_l"].shape[0]
        want = o.compute_cost_volume(g["fl"], g["fr"], D)
        got = vr.compute_cost_volume_vertical(g["fl"], g["fr"], D, 0)
        assert_bits(got[0], want[0], "%s left" % name)
        assert_bits(got[1], want[1], "%s right" % name)
        assert_bits(got[0], g["cv_l"], "%s left against the golden volume" % name)


@pytest.mark.parametrize("H,W,D,seed", [(3, 37, 11, 0), (5, 23, 21, 1)])
def test_restatement_at_range_0_equals_the_oracle_on_ragged_shapes(H, W, D, seed):
    import oracle as o
    rng = np.random.RandomState(seed)
    fl, fr = (rng.standard_normal((H, W, 64)).astype(np.float32) for _ in range(2))
    want = o.compute_cost_volume(fl, fr, D)
    got = vr.compute_cost_volume_vertical(fl, fr, D, 0)
    assert_bits(got[0], want[0], "left")
    assert_bits(got[1], want[1], "right")


def test_restatement_follows_the_definition_pixel_by_pixel():
    """A scalar loop over the definition on a tiny shape: both views, skipped rows, the right view's row h - k."""
    rng = np.random.RandomState(3)
    H, W, D, r = 4, 9, 3, 2
    fl, fr = (rng.standard_normal((H, W, 64)).astype(np.float32) for _ in range(2))
    sl, sr = vr.scores(fl, fr, D, r)

    def p(hl, wl, hr, wr):
        return np.sum(fl[hl, wl] * fr[hr, wr], dtype=np.float32)

    for d in range(D):
        for h in range(H):
            for w in range(d, W):
                assert sl[d, h, w] == max(p(h, w, h + k, w - d) for k in range(-r, r + 1) if 0 <= h + k < H)
            for w in range(W - d):
                assert sr[d, h, w] == max(p(h - k, w + d, h, w) for k in range(-r, r + 1) if 0 <= h - k < H)


def test_restatement_keeps_nan_and_the_first_of_equal_values():
    best, seen = np.zeros((1, 4), np.float32), np.zeros(1, bool)
    nan = np.float32("nan")
    for s in ([-0.0, 1.0, nan, 2.0], [0.0, nan, 5.0, 2.0], [-1.0, 3.0, 7.0, 1.0]):
        vr._take(best, seen, slice(0, 1), np.array([s], np.float32))
    assert np.signbit(best[0, 0]) and best[0, 0] == 0        # -0.0 was first; +0.0 is not larger
    assert np.isnan(best[0, 1]) and np.isnan(best[0, 2])    # a NaN candidate, early or late, stays
    assert best[0, 3] == 2.0


def test_shift_rows_moves_the_image_down_and_repeats_the_edge():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert np.array_equal(vr.shift_rows(a, 2), a[[0, 0, 0, 1]])
    assert np.array_equal(vr.shift_rows(a, -1), a[[1, 2, 3, 3]])
    assert np.array_equal(vr.shift_rows(a, 0), a)


# ---- the entry point: validation before any launch -------------------------------------------------------------------
class _Args(object):
    """A valid call of mccnn_cost_volume_vertical_hwd on fake addresses (nothing is dereferenced before validation ends;
    every case below fails it)."""

    def __init__(self, hip, H=4, W=12, C=64, D=8, r=2):
        self.lib, self.hip = hip.load(), hip
        self.H, self.W, self.C, self.D, self.r = H, W, C, D, r
        self.ptr = dict(fl=0x10000000, fr=0x20000000, lcv=0x30000000, rcv=0x40000000)

    def call(self, null=None):
        p = dict((k, None if k == null else ctypes.c_void_p(v)) for k, v in self.ptr.items())
        rc = self.lib.mccnn_cost_volume_vertical_hwd(p["fl"], p["fr"], self.H, self.W, self.C, self.D, self.r, p["lcv"],
                                                     p["rcv"], None)
        return rc, self.lib.mccnn_last_error_string().decode()


@pytest.fixture(scope="module")
def hip():
    import _hipabi
    _hipabi.load()
    return _hipabi


def test_entry_refuses_null_pointers(hip):
    for name in ("fl", "fr", "lcv", "rcv"):
        rc, msg = _Args(hip).call(null=name)
        assert rc == hip.MCCNN_E_INVALID and "null pointer" in msg, (name, rc, msg)


@pytest.mark.parametrize("r", [-1, 5])
def test_entry_refuses_a_range_outside_0_to_4(hip, r):
    rc, msg = _Args(hip, r=r).call()
    assert rc == hip.MCCNN_E_INVALID and "vertical_range=%d" % r in msg and "[0, 4]" in msg, (rc, msg)


@pytest.mark.parametrize("D", [0, 1, 1025])
def test_entry_refuses_disparity_counts_outside_2_to_1024(hip, D):
    rc, msg = _Args(hip, W=2000, D=D).call()
    assert rc == hip.MCCNN_E_UNSUPPORTED and "D=%d" % D in msg and "[2, 1024]" in msg, (rc, msg)


def test_entry_refuses_more_disparities_than_the_width_allows(hip):
    rc, msg = _Args(hip, W=12, D=11).call()
    assert rc == hip.MCCNN_E_UNSUPPORTED and "W >= D+2" in msg, (rc, msg)
    rc, msg = _Args(hip, C=112).call()
    assert rc == hip.MCCNN_E_UNSUPPORTED and "64 channels" in msg, (rc, msg)


def test_abi_version_is_unchanged_and_the_symbol_is_in_the_table(hip):
    assert hip.load().mccnn_version() == 7 == hip.MCCNN_ABI_VERSION
    assert "mccnn_cost_volume_vertical_hwd" in hip.SIGNATURES


# ---- the flag, the extra and the switch ------------------------------------------------------------------------------
BASE = ["--list_file", "l", "--data_dir", "d", "--save_dir", "s", "-t", "t", "-s", "0", "-e", "0"]


def test_match_parser_accepts_vertical_range_and_it_defaults_to_0():
    import match
    assert match.parser.parse_args(BASE).vertical_range == 0
    assert match.parser.parse_args(BASE + ["--vertical_range", "2"]).vertical_range == 2
    every = BASE + ["--vertical_range", "1", "--views", "both", "--confidence", "msm", "--evaluate", "--paper_sgm",
                    "--pairs_in_flight", "2", "--pipeline", "--dataset", "kitti2015"]
    assert match.parser.parse_args(every).vertical_range == 1


@pytest.mark.parametrize("extra,reason", [(["--fast"], "--fast"), (["--fast", "--separable_cbca"], "--fast"),
                                          (["--separable_cbca"], "--separable_cbca"),
                                          (["--arch", "accurate"], "--arch accurate"),
                                          (["--paper_support_regions"], "--paper_support_regions")])
def test_match_refuses_vertical_range_with_what_has_no_vertical_search(extra, reason, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + ["--vertical_range", "2"] + extra)
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert "--vertical_range is not available with %s" % reason in err, err


@pytest.mark.parametrize("value", ["-1", "5"])
def test_match_refuses_a_range_outside_0_to_4(value, capsys):
    import match
    with pytest.raises(SystemExit) as e:
        match.main(BASE + ["--vertical_range", value])
    assert e.value.code != 0 and "outside [0, 4]" in capsys.readouterr().err


class _StubNet(object):
    def supports_split_features(self):
        return True


class _StubAccurateNet(object):
    fc_weights = ()

    def supports_split_features(self):
        return False


@pytest.fixture
def sd(monkeypatch):
    import torch
    import stereo_device
    monkeypatch.setattr(stereo_device.hip, "require_device", lambda: torch.device("cpu"))
    return stereo_device


def test_matcher_extra_defaults_to_0_and_changes_no_route(sd):
    m = sd.StereoMatcher(_StubNet())
    assert m.extras["vertical_range"] == 0
    v = sd.StereoMatcher(_StubNet(), extras=dict(vertical_range=2))
    assert v.extras["vertical_range"] == 2
    assert v.pixel_major() == m.pixel_major() and v.route(40, 48, 16) == m.route(40, 48, 16)
    assert sd.workspace_bytes(40, 48, 16, v.pixel_major(), v.workspace_cbca_kernel(40, 48, 16)) == \
        sd.workspace_bytes(40, 48, 16, m.pixel_major(), m.workspace_cbca_kernel(40, 48, 16))
    # with everything downstream that the default route offers
    sd.StereoMatcher(_StubNet(), hp=dict(cbca_distance=32), confidence=("msm",), views="both", semi_dense="lr",
                     extras=dict(vertical_range=4, sgm_independent_directions=True))
    with pytest.raises(ValueError, match="unknown extras"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical=2))


@pytest.mark.parametrize("value", [-1, 5, 1.5, True, "2"])
def test_matcher_refuses_a_range_that_is_no_integer_in_0_to_4(sd, value):
    with pytest.raises(ValueError, match=r"vertical_range must be an integer in \[0, 4\]"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_range=value))


def test_matcher_refuses_the_configurations_without_a_vertical_search(sd):
    ex = dict(vertical_range=1)
    with pytest.raises(ValueError, match="accurate network"):
        sd.StereoMatcher(_StubAccurateNet(), extras=ex)
    with pytest.raises(ValueError, match="MCCNN_CV_MFMA"):
        sd.StereoMatcher(_StubNet(), cv_mode=sd.hip.MCCNN_CV_MFMA, extras=ex)
    with pytest.raises(ValueError, match="starts plane-major"):
        sd.StereoMatcher(_StubNet(), layout="plane_major", extras=ex)
    with pytest.raises(ValueError, match="starts plane-major"):
        sd.StereoMatcher(_StubNet(), cbca_order=sd.hip.MCCNN_CBCA_SEPARABLE, extras=ex)
    with pytest.raises(ValueError, match="starts plane-major"):
        sd.StereoMatcher(_StubNet(), extras=dict(vertical_range=1, both_view_support=True))
    # range 0 asks for nothing: all of them stand
    sd.StereoMatcher(_StubAccurateNet(), extras=dict(vertical_range=0))
    sd.StereoMatcher(_StubNet(), cv_mode=sd.hip.MCCNN_CV_MFMA, layout="plane_major", extras=dict(vertical_range=0))


def test_module_switch_exists_and_is_0():
    import process_functional as pf
    import stereo_device
    assert pf.VERTICAL_RANGE == 0
    assert stereo_device.VERTICAL_RANGE_MAX == 4


# ---- why: pairs whose right image sits two rows low ------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,seed", [(96, 128, 32, 0), (96, 128, 32, 1), (128, 192, 48, 2)])
def test_vertical_range_recovers_a_pair_that_is_two_rows_off(net_layers, H, W, D, seed):
    """The whole pipeline on the CPU checker, trained weights, default hyper-parameters, the paper's SGM: the share of
    final pixels within 1 px of the truth (four top and bottom rows left out).  With the right image moved down two rows
    the plain matcher loses 14 to 21 points and a vertical range of 2 brings back all but 2 to 3 of them (measured
    margins between the asserted pairs: 12 to 20 points).  Only the orderings are asserted; what the option costs on
    the aligned pair (0.4 to 2.6 points) is printed."""
    import oracle as o
    import synthetic
    L, R, _, _, truth = synthetic.make_pair(H, W, D, seed=seed)
    truth = np.asarray(truth, np.float64).reshape(H, W)
    fl = o.net_features(L, net_layers)

    def share(right, r):
        fr = o.net_features(right, net_layers)
        cv = o.compute_cost_volume(fl, fr, D) if r == 0 else vr.compute_cost_volume_vertical(fl, fr, D, r)
        return vr.within_1px(ps.match_from_cost_volumes(L, right, cv[0], cv[1], D, True), truth)

    aligned = dict((r, share(R, r)) for r in (0, 1, 2))
    moved = vr.shift_rows(R, 2)
    off = dict((r, share(moved, r)) for r in (0, 2))
    print("%dx%dx%d seed %d: aligned %.3f (range 1: %.3f, range 2: %.3f); two rows off %.3f -> range 2: %.3f"
          % (H, W, D, seed, aligned[0], aligned[1], aligned[2], off[0], off[2]))
    assert off[2] > off[0], (aligned, off)
    assert off[0] < aligned[0], (aligned, off)
