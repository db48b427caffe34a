"""GPU: the mirrored kernels through the C interface and the device wrappers, bit for bit (helpers.assert_bits) against
the left-view restatements applied to flipped arrays (tests/right_view_reference.py; test_right_view_cpu.py pins those
to the rule in image coordinates).

Shapes (H, W, D), right_view_reference.SHAPES: degenerate ones; 31 / 32 / 33 columns (the 32-bit word of the status
kernel's hit mask); 63 / 64 / 65 (ballot and 64-bit word seams of the row kernel); 255 / 256 / 257 (the 256-thread
stride); D > W; D = 1024; 16385 columns (lr_status_walk_kernel, and the per-pixel walk of the interpolation: the row
kernels stop at 16384).  Maps: post_reference.make_lr_maps with the roles swapped, match shares 0.03 / 0.5 / 0.97, with
and without the values the header routes to an occlusion.  Every output is followed by a canary row."""
import numpy as np
import pytest
import torch

import confidence_reference as cr
import right_view_reference as rv
from helpers import assert_bits, module_setting

pytestmark = pytest.mark.gpu

SHAPE_IDS = [rv.shape_id(s) for s in rv.SHAPES]
CANARY_F = np.float32(-12345.0)
CANARY_I = np.int32(-77)
MASKS = [cr.MSM, cr.MMN, cr.CUR, cr.LRC, 15]


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()       # (the cases are handed out read-only)


def status_on_device(dr, dl, D):
    """mccnn_lr_status_right into the first H rows of an (H + 1)-row buffer; the last row is the canary."""
    import stereo_device as sd
    H, W = dr.shape
    buf = torch.full((H + 1, W), int(CANARY_I), dtype=torch.int32, device="cuda")
    got = sd.lr_status_right(dev(dr), dev(dl), D, out=buf[:H])
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert (host[H] == CANARY_I).all(), "the row behind the status map was written"
    return host[:H]


def interpolate_on_device(dr, st, directions, occ):
    import stereo_device as sd
    H, W = dr.shape
    buf = torch.full((H + 1, W), float(CANARY_F), dtype=torch.float32, device="cuda")
    got = sd.interpolate_right(dev(dr), dev(st), out=buf[:H], directions=directions, occlusion_from_right=occ)
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert (host[H] == CANARY_F).all(), "the row behind the interpolated map was written"
    return host[:H]


@pytest.mark.parametrize("si", range(len(rv.SHAPES)), ids=SHAPE_IDS)
def test_status_mask_and_walk_kernels(si):
    """W <= 16384: lr_status_kernel<MIRROR> (hit mask in LDS); 16385: lr_status_walk_kernel<MIRROR>."""
    H, W, D = rv.SHAPES[si]
    n = 0
    for mi, special, dr, dl, want in rv.lr_cases(si):
        what = "%s match %s special %s" % (rv.SHAPES[si], rv.MATCH_SHARES[mi], special)
        if rv.all_states_expected(si):
            assert all((want == v).any() for v in (0, 1, 2)), what + ": a state is missing from the expected map"
        got = status_on_device(dr, dl, D)
        assert got.dtype == want.dtype and np.array_equal(got, want), \
            "%s: %d of %d status words differ" % (what, int((got != want).sum()), want.size)
        n += 1
    assert n == 6


@pytest.mark.parametrize("si", range(len(rv.SHAPES)), ids=SHAPE_IDS)
def test_interpolation_four_modes(si):
    H, W, _ = rv.SHAPES[si]
    n = 0
    for kind in rv.status_kinds_for(W):
        ki = rv.STATUS_KINDS.index(kind)
        for mi in rv.map_kinds_for(W):
            dr, st = rv.interp_inputs(si, ki, mi)
            for directions, occ in rv.MODES:
                got = interpolate_on_device(dr, st, directions, occ)
                assert_bits(got, rv.interp_expected(si, ki, mi, directions, occ),
                            "%s %s %s (%d, %d)" % (rv.SHAPES[si], kind, rv.MAP_KINDS[mi], directions, occ))
                n += 1
    assert n >= 6 * 1 * 4


def test_all_unmatched_rows_wider_than_the_restatement_walks():
    """The kinds right_view_reference leaves out above 300 columns, where their expectation needs no walk: without a
    single match nothing can be filled - every mode returns the raw map - and with a single match in a row the whole
    row's mismatches and the occlusions on its far side take that value."""
    for si in (rv.SHAPES.index((1, 1030, 1024)), rv.SHAPES.index((1, 16385, 4))):
        H, W, _ = rv.SHAPES[si]
        dr, _ = rv.interp_inputs(si, 0, 0)
        st = np.ones((H, W), np.int32)
        st[:, 1::3] = 2
        for directions, occ in rv.MODES:
            assert_bits(interpolate_on_device(dr, st, directions, occ), dr, "all unmatched %d (%d, %d)" % (W, directions, occ))
        for col in (0, W - 1):
            one = st.copy()
            one[0, col] = 0
            value = np.float32(0.0) + dr[0, col]                   # np.median of one value
            for directions, occ in rv.MODES:
                want = dr.copy()
                fill_from_right = bool(occ)
                reaches = (col > np.arange(W)) if fill_from_right else (col < np.arange(W))
                want[0, (one[0] == 2) & reaches] = dr[0, col]
                want[0, one[0] == 1] = value
                assert_bits(interpolate_on_device(dr, one, directions, occ), want,
                            "single match at column %d of %d (%d, %d)" % (col, W, directions, occ))


def test_refusals_with_device_pointers():
    import _hipabi as hip
    lib = hip.load()
    H, W = 4, 70
    dr = torch.zeros((H, W), device="cuda")
    st = torch.ones((H, W), dtype=torch.int32, device="cuda")
    out = torch.zeros((H, W), device="cuda")
    s = hip.stream()
    for directions, occ in rv.MODES:
        assert lib.mccnn_interpolate_right(hip.ptr(dr), hip.ptr(st), H, W, directions, int(occ), hip.ptr(dr), s) == hip.MCCNN_E_INVALID
        assert b"mccnn_interpolate_right: out must not alias the input map" in lib.mccnn_last_error_string()
        assert lib.mccnn_interpolate_right(hip.ptr(dr), hip.ptr(st), H, W, directions, int(occ), hip.ptr(st), s) == hip.MCCNN_E_INVALID
        assert b"mccnn_interpolate_right: out must not alias the status map" in lib.mccnn_last_error_string()
        assert lib.mccnn_interpolate_right(hip.ptr(dr), hip.ptr(st), H, W, directions, int(occ), hip.ptr(out), s) == 0
    vol = torch.zeros((H, W, 4), device="cuda")
    buf = torch.zeros((5, H, W), device="cuda")
    for fn in (lib.mccnn_confidence_right_hwd, lib.mccnn_confidence_right):
        assert fn(hip.ptr(vol), hip.ptr(buf[1]), 4, H, W, 15, hip.ptr(buf), s) == hip.MCCNN_E_INVALID
        assert b"overlaps disp_left" in lib.mccnn_last_error_string()
        assert fn(hip.ptr(vol), hip.ptr(buf[4]), 4, H, W, 15, hip.ptr(buf), s) == 0
    torch.cuda.synchronize()


def test_drop_in_interpolation_right():
    """process_functional.interpolation_right: NumPy in, NumPy out, INTERPOLATION_DIRECTIONS / OCCLUSION_FROM_LEFT
    honoured (mirrored)."""
    import process_functional as pf
    si = rv.SHAPES.index((4, 70, 64))
    H, W, D = rv.SHAPES[si]
    _, _, dr, dl, status = next(iter(rv.lr_cases(si)))
    for directions, occ in rv.MODES:
        with module_setting(pf, "INTERPOLATION_DIRECTIONS", directions), module_setting(pf, "OCCLUSION_FROM_LEFT", occ):
            got = pf.interpolation_right(dr.copy(), dl.copy(), D)
        assert isinstance(got, np.ndarray)
        assert_bits(got, rv.interpolate_right(dr, status, directions, occ), "interpolation_right (%d, %d)" % (directions, occ))


# ---- confidence -----------------------------------------------------------------------------------------------------
def run_confidence(entry, vol, D, left, mask):
    """One launch into the first K planes of a K + 1 plane buffer; the last plane is the canary."""
    import stereo_device as sd
    k = bin(mask).count("1")
    H, W = left.shape
    buf = torch.full((k + 1, H, W), float(CANARY_F), dtype=torch.float32, device="cuda")
    dl = left if mask & cr.LRC else None
    if entry == "hwd":
        got = sd.confidence_right_hwd(vol, D, dl, rv.names_of(mask), out=buf[:k])
    else:
        got = sd.confidence_right(vol, dl, rv.names_of(mask), out=buf[:k])
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert (host[k] == CANARY_F).all(), "the plane behind the %d requested ones was written" % k
    return host[:k]


@pytest.mark.parametrize("ci", range(len(rv.CONF_SHAPES)), ids=[rv.shape_id(s) for s in rv.CONF_SHAPES])
@pytest.mark.parametrize("ki", range(len(rv.CONF_KINDS)), ids=rv.CONF_KINDS)
def test_confidence_right_both_layouts(ci, ki):
    """Pad lanes poisoned with -inf on one run and NaN on another; single measures reproduce their plane of the all-four
    run; the last column's winners look past the image (x + d1 > W-1: -inf)."""
    H, W, D = rv.CONF_SHAPES[ci]
    vol, left, want, d1 = rv.conf_case(ci, ki)
    last = d1[:, W - 1]
    assert (last > 0).any() and (want[3][:, W - 1][last > 0] == -np.inf).all()
    dleft, dvol = dev(left), dev(vol)
    for pad in (-np.inf, np.nan):
        hwd = dev(cr.to_hwd(vol, pad))
        for mask in MASKS:
            assert_bits(run_confidence("hwd", hwd, D, dleft, mask), rv.planes_of(want, mask),
                        "mccnn_confidence_right_hwd %s %s pad %s measures %d" % (rv.CONF_SHAPES[ci], rv.CONF_KINDS[ki], pad, mask))
    for mask in MASKS:
        assert_bits(run_confidence("dhw", dvol, D, dleft, mask), rv.planes_of(want, mask),
                    "mccnn_confidence_right %s %s measures %d" % (rv.CONF_SHAPES[ci], rv.CONF_KINDS[ki], mask))


def test_drop_in_confidence_view_right():
    import process_functional as pf
    vol, left, want, _ = rv.conf_case(rv.CONF_SHAPES.index((7, 11, 16)), 0)
    vol, left = vol.copy(), left.copy()
    got = pf.confidence_measures(vol, left, ("lrc", "msm"), view="right")
    assert sorted(got) == ["lrc", "msm"]
    assert_bits(got["msm"], want[0], "msm")
    assert_bits(got["lrc"], want[3], "lrc")
    with pytest.raises(ValueError):
        pf.confidence_measures(vol, left, ("msm",), view="both")
