"""CPU: what the right view promises without a GPU.

  * the flip identity: the rule of include/mccnn.h spelled out in image coordinates (right_view_reference's literal
    loops: partner at x + d, candidates d < min(W - x, D), occlusions from the left, rays whose columns round half DOWN)
    equals the left-view restatements applied to the flipped arrays, on every case the GPU tests use;
  * the inputs are what the GPU tests need: all three states occur in every expected status map of 12 pixels or more;
  * header, library and binding carry the four entry points, and each refuses bad arguments before any HIP call;
  * workspace_bytes(views="left") is what it was, views="both" adds the right view's planes;
  * match.py knows --views and refuses it for the KITTI layouts."""
import ctypes
import os

import numpy as np
import pytest

import confidence_reference as cr
import right_view_reference as rv
from helpers import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
NEW = ("mccnn_lr_status_right", "mccnn_interpolate_right", "mccnn_confidence_right_hwd", "mccnn_confidence_right")
SHAPE_IDS = [rv.shape_id(s) for s in rv.SHAPES]


@pytest.mark.parametrize("si", range(len(rv.SHAPES)), ids=SHAPE_IDS)
def test_status_loop_equals_the_flipped_restatement(si):
    H, W, D = rv.SHAPES[si]
    for mi, special, dr, dl, want in rv.lr_cases(si):
        what = "%s match %s special %s" % (rv.SHAPES[si], rv.MATCH_SHARES[mi], special)
        if rv.all_states_expected(si):
            assert all((want == v).any() for v in (0, 1, 2)), what + ": a state is missing from the expected map"
        got = rv.lr_status_right_loop(dr, dl, D)
        assert got.dtype == want.dtype and np.array_equal(got, want), what


@pytest.mark.parametrize("si", range(len(rv.SHAPES)), ids=SHAPE_IDS)
def test_interpolation_loop_equals_the_flipped_restatement(si):
    H, W, _ = rv.SHAPES[si]
    n = 0
    for kind in rv.status_kinds_for(W):
        ki = rv.STATUS_KINDS.index(kind)
        for mi in rv.map_kinds_for(W):
            dr, st = rv.interp_inputs(si, ki, mi)
            for directions, occ in rv.MODES:
                want = rv.interp_expected(si, ki, mi, directions, occ)
                got = rv.interpolate_right_loop(dr, st, directions, occ)
                assert_bits(got, want, "%s %s %s (%d, %d)" % (rv.SHAPES[si], kind, rv.MAP_KINDS[mi], directions, occ))
                n += 1
    assert n >= 6 * 1 * 4


def test_single_matches_sit_in_the_first_and_last_column():
    si = rv.SHAPES.index((3, 65, 16))
    for kind, col in (("corner_match", 64), ("first_column_match", 0)):
        _, st = rv.interp_inputs(si, rv.STATUS_KINDS.index(kind), 0)
        ys, xs = np.nonzero(st == 0)
        assert len(xs) == 1 and xs[0] == col, kind
    _, st = rv.interp_inputs(si, rv.STATUS_KINDS.index("all_mismatch"), 0)
    assert (st != 0).all()
    _, st = rv.interp_inputs(si, rv.STATUS_KINDS.index("odd_words"), 0)
    assert np.isin(st, (3, -1, 7)).any()


def test_half_down_columns_differ_from_a_naive_copy():
    """The 16-ray rule must not be the left kernel's rounding with the rays turned round: on a checkerboard of matches a
    half step lands on another pixel.  (A guard for the restatement, not a bound on the kernel.)"""
    import math
    w, dx = 10, -0.5        # the image-frame step of the flipped frame's ray (0.5, 1)
    assert int(math.ceil(w + 1 * dx - 0.5)) == 9 and int(math.floor(w + 1 * dx + 0.5)) == 10
    si = rv.SHAPES.index((4, 70, 64))
    ki = rv.STATUS_KINDS.index("checkerboard")
    dr, st = rv.interp_inputs(si, ki, 0)
    want = rv.interp_expected(si, ki, 0, 16, False)
    import paper_rules_reference as ppr
    naive = ppr.interpolate_ex(dr, st, 16, True)       # the left rule on the unflipped map, occlusions from the left
    assert not np.array_equal(naive.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("ci", range(len(rv.CONF_SHAPES)), ids=[rv.shape_id(s) for s in rv.CONF_SHAPES])
def test_confidence_right_is_the_left_rule_with_x_plus_d1(ci):
    H, W, D = rv.CONF_SHAPES[ci]
    for ki, kind in enumerate(rv.CONF_KINDS):
        vol, left, planes, d1 = rv.conf_case(ci, ki)
        # MSM, MMN and CUR: the unchanged definitions on the right volume (no flip at all)
        same, d1_same = cr.confidence(vol, None, 7)
        assert np.array_equal(d1, d1_same)
        assert_bits(planes[:3], same, "%s %s MSM/MMN/CUR" % (rv.CONF_SHAPES[ci], kind))
        assert_bits(planes[3], rv.lrc_right_loop(d1, left), "%s %s LRC" % (rv.CONF_SHAPES[ci], kind))
        last = d1[:, W - 1]
        assert (planes[3][:, W - 1][last > 0] == -np.inf).all() and (last > 0).any()     # x + d1 > W-1
        if H * W >= 60:
            assert (d1 == -1).any() and (d1 == 0).any() and (d1 == D - 1).any()
            assert np.isfinite(planes[3]).any() and (planes[3] == 0).any()


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_declared_bound_and_exported():
    import _hipabi
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    lib = _hipabi.load()
    for name in NEW:
        assert "int %s(" % name in text and name in _hipabi.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.mccnn_version() == 7


def test_argument_refusals():
    import _hipabi
    lib = _hipabi.load()
    a, b, c = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x500000), ctypes.c_void_p(0x900000)

    def msg():
        return lib.mccnn_last_error_string()

    fn = lib.mccnn_lr_status_right
    for args in ((None, b, 4, 6, 3, c), (a, None, 4, 6, 3, c), (a, b, 4, 6, 3, None)):
        assert fn(*args, None) == E_INVALID and b"mccnn_lr_status_right: null pointer" in msg()
    for H, W, D in ((0, 6, 3), (4, 0, 3), (4, 6, 0), (-1, 6, 3)):
        assert fn(a, b, H, W, D, c, None) == E_INVALID and b"non-positive" in msg()
    assert fn(a, b, 65536, 16385, 3, c, None) == E_UNSUPPORTED and b"H=65536" in msg()

    fn = lib.mccnn_interpolate_right
    for args in ((None, b, 4, 6, 4, 0, c), (a, None, 4, 6, 4, 0, c), (a, b, 4, 6, 4, 0, None)):
        assert fn(*args, None) == E_INVALID and b"mccnn_interpolate_right: null pointer" in msg()
    for H, W in ((0, 6), (4, 0), (4, -2)):
        assert fn(a, b, H, W, 4, 0, c, None) == E_INVALID and b"non-positive" in msg()
    for directions, occ in ((4, 0), (4, 1), (16, 0), (16, 1)):
        assert fn(a, b, 4, 6, directions, occ, a, None) == E_INVALID and b"alias the input map" in msg()
        assert fn(a, b, 4, 6, directions, occ, b, None) == E_INVALID and b"alias the status map" in msg()
        assert fn(a, b, 65536, 6, directions, occ, c, None) == E_UNSUPPORTED and b"H=65536" in msg()
    for directions in (0, 8, 5, -4):
        assert fn(a, b, 4, 6, directions, 0, c, None) == E_INVALID and b"directions" in msg()

    vol, left, out = a, b, c
    for fn, who in ((lib.mccnn_confidence_right_hwd, b"mccnn_confidence_right_hwd"),
                    (lib.mccnn_confidence_right, b"mccnn_confidence_right")):
        assert fn(None, left, 8, 4, 6, 15, out, None) == E_INVALID and b"null pointer" in msg() and who in msg()
        assert fn(vol, left, 8, 4, 6, 15, None, None) == E_INVALID and b"null pointer" in msg()
        for D in (1, 0, -3):
            assert fn(vol, left, D, 4, 6, 15, out, None) == E_INVALID and b"two disparities" in msg()
        for H, W in ((0, 6), (4, 0), (-1, 6), (4, -1)):
            assert fn(vol, left, 8, H, W, 15, out, None) == E_INVALID and b"non-positive" in msg()
        for measures in (0, 16, 17, 32, 0x80000000):
            assert fn(vol, left, 8, 4, 6, measures, out, None) == E_INVALID and b"measures" in msg()
        for measures in (8, 9, 15):
            assert fn(vol, None, 8, 4, 6, measures, out, None) == E_INVALID and b"disp_left" in msg()
        plane = 4 * 6 * 4
        for k, measures in ((1, 1), (2, 3), (4, 15)):
            for r in (out.value, out.value + 4, out.value + k * plane - 4, out.value - plane + 4):
                assert fn(vol, ctypes.c_void_p(r), 8, 4, 6, measures, out, None) == E_INVALID and b"overlaps" in msg()
    assert lib.mccnn_confidence_right_hwd(vol, left, 1025, 4, 6, 15, out, None) == E_UNSUPPORTED and b"1024" in msg()
    assert lib.mccnn_confidence_right_hwd(vol, None, 4096, 4, 6, 7, out, None) == E_UNSUPPORTED


# ---- host layers ------------------------------------------------------------------------------------------------------
def test_workspace_bytes_by_view():
    """views="left" is the value tests/test_large_envelope_cpu.py states at its shapes; "both" adds one status plane,
    three maps, the [2,H,W] result and a second set of confidence planes."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    for H, W, D, dp in ((1988, 2880, 800, 800), (12, 1100, 1022, 1024)):
        today = 4 * H * W * dp * 4 + (5 * lib.mccnn_sgm_scratch_bytes(H, W, D) + 2 * lib.mccnn_support_bytes(H, W)
                                      + 7 * H * W * 4 + 2 * lib.mccnn_cbca_prog_bytes(D, H, W))
        assert sd.workspace_bytes(H, W, D) == today == sd.workspace_bytes(H, W, D, views="left")
        assert sd.workspace_bytes(H, W, D, views="both") == today + 6 * H * W * 4
        for k in (1, 4):
            assert sd.workspace_bytes(H, W, D, confidence=k, views="left") == today + k * H * W * 4
            assert sd.workspace_bytes(H, W, D, confidence=k, views="both") == today + (6 + 2 * k) * H * W * 4
        assert sd.workspace_bytes(H, W, D, pairs_in_flight=3, views="both") == 3 * (today + 6 * H * W * 4)
    assert 103e9 < sd.workspace_bytes(2048, 3072, 1024, views="left") < 104e9
    with pytest.raises(ValueError, match="views"):
        sd.workspace_bytes(12, 1100, 64, views="right")


def test_match_knows_the_flag_and_refuses_it_for_kitti(tmp_path, capsys):
    import match
    assert match.right_gt_suffix == "disp1GT.pfm"
    assert "--views" in match.parser.format_help()
    listing = tmp_path / "list.txt"
    listing.write_text("")
    for dataset in ("kitti2012", "kitti2015"):
        with pytest.raises(SystemExit) as e:
            match.main(["--list_file", str(listing), "--data_dir", str(tmp_path), "--save_dir", str(tmp_path), "-t", "x",
                        "-s", "0", "-e", "0", "--dataset", dataset, "--views", "both"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--views both" in err and "right-view" in err and "submission" in err
