"""GPU: every kernel of csrc/post.hip (a7-a11) and the region list of a3 at their edges, against the literal NumPy
reference of tests/post_reference.py and - where the literal's Python loops are too slow (rows wider than 16384,
65535 rows) - against the CPU oracle, which test_post_edges_cpu.py pins to the literal on the same kinds of input.
uint32 comparison throughout (helpers.assert_bits / bits_strict); no pixel and no case is left out.

kernel -> test
  wta_kernel, mccnn_wta_hwd                    test_wta_and_its_pixel_major_twin
  subpixel_kernel<false>, mccnn_subpixel_hwd   test_subpixel_and_its_pixel_major_twin, test_no_winner_map_...
  lr_status_kernel                             test_lr_status_and_interpolation_small_maps, ..._wide_rows (W = 16384)
  lr_status_walk_kernel                        test_lr_status_and_interpolation_wide_rows (W = 16385, 20000)
  interpolate_vertical_kernel / _row_kernel    ..._small_maps, ..._wide_rows (16384), ..._tall_columns (H = 65534)
  interpolate_kernel                           ..._wide_rows (16385, 20000), ..._tall_columns (H = 65535)
  median_kernel, median5x5_kernel              test_median_matrix, test_filters_across_a_block_boundary
  bilateral_kernel, bilateral5x5_kernel        test_bilateral_matrix, test_filters_across_a_block_boundary
  cross_region_list_kernel                     test_region_list_every_slot
  interpolate_paper_kernel                     test_paper_rules_gpu.py::test_paper_interpolation
  subpixel_kernel<true>, subpixel_hwd<true>    test_paper_rules_gpu.py::test_numpy1_subpixel
(the two opt-in extras: their edges are in test_paper_rules_gpu.py, against tests/paper_rules_reference.py; a NaN
neighbour in median_upto4, which no mccnn_lr_status map produces, is there too.)"""
import numpy as np
import pytest
import torch

import post_reference as ref
from helpers import _describe, assert_bits, bits_strict

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def settle(failures, total, what):
    assert not failures, "%s: %d of %d cases differ:\n%s" % (what, len(failures), total, "\n".join(failures[:40]))


# ---- a10 / a11 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wi", range(len(ref.WINDOWS)), ids=["%dx%d" % w for w in ref.WINDOWS])
def test_median_matrix(wi):
    """The shape x window x value-class matrix of the CPU file through the drop-in (process_functional.median_filter):
    images smaller than the window, the H >= 5 && W >= 5 boundary of the 5x5 kernel, every clipped tap count."""
    import process_functional as pf
    fh, fw = ref.WINDOWS[wi]
    failures, total = [], 0
    for shape, kind, m in ref.median_cases(wi):
        total += 1
        got, want = pf.median_filter(m, fh, fw), ref.median_filter(m, fh, fw)
        if not bits_strict(got, want):
            failures.append("median %dx%d on %s %s: %s" % (fh, fw, shape, kind, _describe(got, want)))
    settle(failures, total, "median %dx%d" % (fh, fw))


@pytest.mark.parametrize("wi", range(len(ref.WINDOWS)), ids=["%dx%d" % w for w in ref.WINDOWS])
def test_bilateral_matrix(wi):
    import process_functional as pf
    fh, fw = ref.WINDOWS[wi]
    failures, total = [], 0
    for shape, kind, img, m in ref.bilateral_cases(wi):
        for sigma, thr in ref.BILATERAL_SETTINGS:
            total += 1
            got = pf.bilateral_filter(img[:, :, None], m, fh, fw, 0, sigma, thr)
            want = ref.bilateral_filter(img, m, fh, fw, 0, sigma, thr)
            if not bits_strict(got, want):
                failures.append("bilateral %dx%d sigma %g thr %g on %s %s: %s"
                                % (fh, fw, sigma, thr, shape, kind, _describe(got, want)))
    settle(failures, total, "bilateral %dx%d" % (fh, fw))


@pytest.mark.parametrize("W", [255, 256, 257, 600])
def test_filters_across_a_block_boundary(W):
    """Rows that end just before, at and just behind a 256-thread block, and rows of several blocks, at H = 6: both 5x5
    kernels (which have interior and border pixels here) and both generic ones, special values in both kinds of pixel."""
    import stereo_device as sd
    H = 6
    rng = ref.case_rng(6, W)
    m = ref.make_map((H, W), "special", rng)
    img = ref.make_image((H, W), "special", rng)
    specials = [np.nan, np.inf, -np.inf, -0.0, -1.0]
    for k, v in enumerate(specials):                     # interior pixels of the 5x5 window (rows 2..3, columns 2..W-3)
        m[2 + k % 2, 3 + 7 * k] = v
        m[2 + (k + 1) % 2, W - 4 - 5 * k] = v
    for k, v in enumerate(specials):                     # border pixels: first / last rows and columns, block seams
        m[0, 11 * k] = v
        m[H - 1, W - 1 - 3 * k] = v
        m[k % H, 0] = v
    m[1, min(W - 1, 255)] = -0.0
    m[4, min(W - 1, 256)] = np.nan
    img[3, W // 2] = np.nan                              # an interior NaN centre pixel besides make_image's
    img[0, W - 1] = np.nan                               # and a border one
    interior = np.zeros((H, W), bool)
    interior[2:H - 2, 2:W - 2] = True
    assert (~np.isfinite(m) & interior).any() and (~np.isfinite(m) & ~interior).any()
    assert (np.signbit(m) & (m == 0) & interior).any() and (np.signbit(m) & (m == 0) & ~interior).any()
    for fh, fw in ((5, 5), (3, 7), (7, 7)):
        got = sd.median(dev(m), fh, fw).cpu().numpy()
        assert_bits(got, ref.median_filter(m, fh, fw), "median %dx%d W=%d" % (fh, fw, W))
        got = sd.bilateral(dev(img), dev(m), fh, fw, 0, 6, 2).cpu().numpy()
        assert_bits(got, ref.bilateral_filter(img, m, fh, fw, 0, 6, 2), "bilateral %dx%d W=%d" % (fh, fw, W))


def test_median_of_negative_zero_is_positive_zero():
    """np.median ends in np.mean, whose float32 sum starts from +0 (all three median routines of post.hip)."""
    import stereo_device as sd
    nz = np.float32(-0.0)
    m = np.full((6, 9), nz, dtype=np.float32)
    for fh, fw in ((1, 1), (5, 5), (3, 3), (1, 3)):               # odd and even clipped counts, 5x5 and generic kernels
        got = sd.median(dev(m), fh, fw).cpu().numpy()
        want = ref.median_filter(m, fh, fw)
        assert not np.signbit(want).any()
        assert_bits(got, want, "median %dx%d of -0.0" % (fh, fw))
    # median_upto4 through the interpolation: mismatches between matches that hold -0.0
    dl = np.array([[nz, 5, nz, 5, nz]], dtype=np.float32)
    st = np.array([[0, 1, 0, 1, 0]], dtype=np.int32)
    got = sd.interpolate(dev(dl), dev(st)).cpu().numpy()
    want = ref.interpolate(dl, st)
    assert not np.signbit(want[0, 1]) and want[0, 1] == 0
    assert_bits(got, want, "interpolation between -0.0 matches")
    assert_bits(sd.interpolate(dev(dl), dev(st), occlusion_from_left=True).cpu().numpy(), want, "paper kernel, same rule")


def test_bilateral_gated_out_taps_still_count():
    """A shut gate multiplies the tap by 0, it does not skip it: 0 * NaN = 0 * inf = NaN, as NumPy computes.  A NaN
    centre pixel shuts every gate of its window and a threshold of 0 shuts every gate anywhere: 0 / 0."""
    import stereo_device as sd
    img = np.zeros((7, 8), dtype=np.float32)
    img[3, 4] = 10                                     # gated out of every neighbour's window (threshold 2)
    for fh, fw in ((3, 3), (5, 5)):
        for bad in (np.nan, np.inf, -np.inf):
            m = np.ones((7, 8), dtype=np.float32)
            m[3, 4] = bad
            want = ref.bilateral_filter(img, m, fh, fw, 0, 6, 2)
            assert np.isnan(want[2:5, 3:6]).sum() >= 8 and np.isfinite(want[0, 0])
            assert_bits(sd.bilateral(dev(img), dev(m), fh, fw, 0, 6, 2).cpu().numpy(), want, "gated-out %r" % bad)
        m = np.arange(56, dtype=np.float32).reshape(7, 8)
        nan_img = img.copy()
        nan_img[3, 4] = np.nan
        want = ref.bilateral_filter(nan_img, m, fh, fw, 0, 6, 2)
        assert np.isnan(want[3, 4]) and np.isfinite(want).sum() == 55
        assert_bits(sd.bilateral(dev(nan_img), dev(m), fh, fw, 0, 6, 2).cpu().numpy(), want, "NaN centre pixel")
        want = ref.bilateral_filter(img, m, fh, fw, 0, 6, 0)
        assert np.isnan(want).all()
        assert_bits(sd.bilateral(dev(img), dev(m), fh, fw, 0, 6, 0).cpu().numpy(), want, "threshold 0")


def _rc(lib, rc, code, text):
    assert rc == code, "returned %d, expected %d (%s)" % (rc, code, lib.mccnn_last_error_string())
    assert text in lib.mccnn_last_error_string(), lib.mccnn_last_error_string()


def test_window_limits():
    """49 taps are served (7x7, 1x49, 49x1 are in the matrices above); 51 taps, even sizes and 0 are refused with
    MCCNN_E_UNSUPPORTED and nothing is launched (the output keeps its canary)."""
    import _hipabi as hip
    lib = hip.load()
    H, W = 6, 9
    m = dev(np.arange(H * W, dtype=np.float32).reshape(H, W))
    tab = dev(np.ones((64,), dtype=np.float32))
    for fh, fw in ((3, 17), (17, 3), (7, 9), (4, 5), (5, 4), (2, 2), (0, 5), (5, 0), (-1, 3), (51, 1)):
        out = torch.full((H, W), -77.0, device="cuda")
        _rc(lib, lib.mccnn_median(hip.ptr(m), H, W, fh, fw, hip.ptr(out), hip.stream()), E_UNSUPPORTED, b"mccnn_median: window")
        _rc(lib, lib.mccnn_bilateral(hip.ptr(m), hip.ptr(m), H, W, fh, fw, hip.ptr(tab), 2.0, hip.ptr(out), hip.stream()),
            E_UNSUPPORTED, b"mccnn_bilateral: window")
        torch.cuda.synchronize()
        assert bool((out == -77.0).all())


def test_rows_beyond_the_grid_are_refused():
    """Rows go on blockIdx.y in the median, the bilateral, the paper-rule and the fallback interpolation kernels (and
    in the left-right walk kernel): 65535 rows are served (test_..._tall_columns), 65536 are MCCNN_E_UNSUPPORTED before
    anything is launched."""
    import _hipabi as hip
    lib = hip.load()
    H, W = 65536, 1
    m = torch.zeros((H, W), device="cuda")
    st = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    tab = torch.ones((25,), device="cuda")
    out = torch.full((H, W), -77.0, device="cuda")
    s = hip.stream()
    _rc(lib, lib.mccnn_median(hip.ptr(m), H, W, 5, 5, hip.ptr(out), s), E_UNSUPPORTED, b"mccnn_median: H=65536")
    _rc(lib, lib.mccnn_median(hip.ptr(m), H, W, 3, 3, hip.ptr(out), s), E_UNSUPPORTED, b"mccnn_median: H=65536")
    _rc(lib, lib.mccnn_bilateral(hip.ptr(m), hip.ptr(m), H, W, 5, 5, hip.ptr(tab), 2.0, hip.ptr(out), s), E_UNSUPPORTED,
        b"mccnn_bilateral: H=65536")
    _rc(lib, lib.mccnn_bilateral(hip.ptr(m), hip.ptr(m), H, W, 3, 3, hip.ptr(tab), 2.0, hip.ptr(out), s), E_UNSUPPORTED,
        b"mccnn_bilateral: H=65536")
    _rc(lib, lib.mccnn_interpolate(hip.ptr(m), hip.ptr(st), H, W, hip.ptr(out), s), E_UNSUPPORTED,
        b"mccnn_interpolate: H=65536")
    _rc(lib, lib.mccnn_interpolate_ex(hip.ptr(m), hip.ptr(st), H, W, 16, 1, hip.ptr(out), s), E_UNSUPPORTED,
        b"mccnn_interpolate_ex: H=65536")
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    # narrow rows of the left-right check go on blockIdx.x: any height is served
    assert lib.mccnn_lr_status(hip.ptr(m), hip.ptr(m), H, W, 4, hip.ptr(st), s) == 0
    torch.cuda.synchronize()
    assert bool((st == 0).all())


def test_status_must_not_alias_out():
    """mccnn_interpolate used to take its slow kernel for status == out, in which other threads still read the status
    words being overwritten; both entry points refuse it now (MCCNN_E_INVALID) and launch nothing."""
    import _hipabi as hip
    lib = hip.load()
    H, W = 5, 9
    dl = dev(np.arange(H * W, dtype=np.float32).reshape(H, W))
    pattern = np.tile(np.array([0, 1, 2], dtype=np.int32), H * W // 3).reshape(H, W)
    st = dev(pattern)
    s = hip.stream()
    _rc(lib, lib.mccnn_interpolate(hip.ptr(dl), hip.ptr(st), H, W, hip.ptr(st), s), E_INVALID,
        b"mccnn_interpolate: out must not alias the status map")
    for directions, left in ((4, 0), (4, 1), (16, 0), (16, 1)):
        _rc(lib, lib.mccnn_interpolate_ex(hip.ptr(dl), hip.ptr(st), H, W, directions, left, hip.ptr(st), s), E_INVALID,
            b"mccnn_interpolate_ex: out must not alias the status map")
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), pattern)
    _rc(lib, lib.mccnn_interpolate(hip.ptr(dl), hip.ptr(st), H, W, hip.ptr(dl), s), E_INVALID, b"alias the input map")


# ---- a8 ---------------------------------------------------------------------------------------------------------------
def test_lr_status_and_interpolation_small_maps():
    """The maps of the CPU file - fractional, >= D, -0.0, -0.5, -1, -3, NaN, -inf on the left; -1, -2, -1.0000001,
    fractional, >= D, NaN, +inf on the right - against the literal, the undefined left values held to the header."""
    import stereo_device as sd
    failures, total, seen = [], 0, set()
    for shape, match, special, dl, dr in ref.lr_cases():
        total += 1
        D = shape[2]
        want_st = ref.lr_status(dl, dr, D)
        seen |= set(np.unique(want_st).tolist())
        st = sd.lr_status(dev(dl), dev(dr), D)
        got_st = st.cpu().numpy()
        assert (got_st[~(dl > -1)] == 2).all()
        if not np.array_equal(got_st, want_st):
            failures.append("lr_status %s match %g special %s: %d differ" % (shape, match, special, (got_st != want_st).sum()))
        got = sd.interpolate(dev(dl), dev(want_st)).cpu().numpy()
        want = ref.interpolate(dl, want_st)
        if not bits_strict(got, want):
            failures.append("interpolation %s match %g special %s: %s" % (shape, match, special, _describe(got, want)))
    assert seen == {0, 1, 2}
    settle(failures, 2 * total, "left-right check and interpolation")


def big_lr_maps(H, W, D, match, rng):
    """Vectorised maps for the shapes the literal is too slow for: the right map is constant per row (so that a left
    pixel holding that constant matches and any other integer is a mismatch) with a stretch of out-of-range values
    (left pixels that look only into it are occlusions), 10 % edge values, and a share `match` of consistent left
    pixels; a column and a row without any match."""
    c = rng.integers(0, D, size=(H, 1))
    dr = np.broadcast_to(c, (H, W)).astype(np.float32).copy()
    noise = rng.random((H, W)) < 0.1
    right_vals = np.array([-1, -2, -1.0000001, 0.5, 1.5, D - 0.5, D, D + 3, np.nan, np.inf], dtype=np.float32)
    dr[noise] = rng.choice(right_vals, size=int(noise.sum()))
    if W > 4 * D:
        dr[:, W // 2:W // 2 + 2 * D] = D + 5
    else:
        dr[H // 3:H // 3 + 50] = D + 5
    dl = np.where(rng.random((H, W)) < match, c, rng.integers(0, D, size=(H, W))).astype(np.float32)
    edge = rng.random((H, W)) < 0.03
    left_vals = np.array([0.5, 1.5, D - 1.5, D - 0.5, D, D + 2, -0.0, -0.5, -1.0, -3.0, np.nan, -np.inf], dtype=np.float32)
    dl[edge] = rng.choice(left_vals, size=int(edge.sum()))
    dl[:, W // 3] = -1                                  # a column without any match
    dl[H // 2, :] = -1                                  # a row without any match
    return dl, dr


def _check_against_oracle(H, W, D, key):
    import oracle as o
    import stereo_device as sd
    for mi, match in enumerate((0.03, 0.5, 0.97)):
        dl, dr = big_lr_maps(H, W, D, match, ref.case_rng(7, key, mi))
        want_st = o.lr_status(dl, dr, D)
        assert set(np.unique(want_st).tolist()) == {0, 1, 2}
        assert (want_st[:, W // 3] != 0).all() and (want_st[H // 2, :] != 0).all()
        ddl = dev(dl)
        st = sd.lr_status(ddl, dev(dr), D)
        assert np.array_equal(st.cpu().numpy(), want_st), "lr_status %dx%d match %g" % (H, W, match)
        got = sd.interpolate(ddl, st).cpu().numpy()
        assert_bits(got, o.interpolation(dl, dr, D), "interpolation %dx%d match %g" % (H, W, match))


@pytest.mark.parametrize("W", [16384, 16385, 20000])
def test_lr_status_and_interpolation_wide_rows(W):
    """W = 16384 is the last width of the mask kernels (lr_status_kernel, interpolate_vertical / _row_kernel); 16385 and
    20000 take lr_status_walk_kernel and interpolate_kernel, which nothing else launches."""
    _check_against_oracle(3, W, 40, W)


@pytest.mark.parametrize("H", [65534, 65535])
def test_lr_status_and_interpolation_tall_columns(H):
    """H = 65534 is the last height whose rows fit the 16-bit row indices of interpolate_vertical_kernel beside the 0xffff
    sentinel; H = 65535 takes interpolate_kernel (and is the last height of its grid)."""
    _check_against_oracle(H, 3, 3, H)


# ---- a7 / a9 ----------------------------------------------------------------------------------------------------------
def test_wta_and_its_pixel_major_twin():
    """D = 1, 2, 3, 5, 7, 12 (the remainder loop), H*W = 1, 255, 256, 257, ties, all-NaN and all-+inf pixels (-1)."""
    import stereo_device as sd
    total = 0
    for vol in ref.wta_volumes():
        total += 1
        D = vol.shape[0]
        want = ref.disparity_prediction_one(vol)
        v = dev(vol)
        assert_bits(sd.wta(v).cpu().numpy(), want, "wta %s" % (vol.shape,))
        assert_bits(sd.wta_hwd(sd.dhw_to_hwd(v), D).cpu().numpy(), want, "wta_hwd %s" % (vol.shape,))
    assert total == 24


def test_subpixel_and_its_pixel_major_twin():
    """Integer, x.5, D - 1.5, D - 1, >= D, -1, -0.0 and -0.5 disparities (both ends of the range), a flat cost curve."""
    import stereo_device as sd
    for shape, d, vol in ref.subpixel_cases():
        D = shape[2]
        want = ref.subpixel_enhance(d, vol)
        v = dev(vol)
        assert_bits(sd.subpixel(dev(d), v).cpu().numpy(), want, "subpixel %s" % (shape,))
        assert_bits(sd.subpixel_hwd(dev(d), sd.dhw_to_hwd(v), D).cpu().numpy(), want, "subpixel_hwd %s" % (shape,))


def test_no_winner_map_through_the_later_stages():
    """A volume without any finite cost gives -1 everywhere; -1 is an occlusion for the left-right check, stays -1
    through the interpolation (no match to copy from) and through the sub-pixel step (int(d - 1) < 0)."""
    import stereo_device as sd
    D, H, W = 5, 4, 9
    vol = np.full((D, H, W), np.nan, dtype=np.float32)
    vol[:, 1] = np.inf
    v = dev(vol)
    for disp in (sd.wta(v), sd.wta_hwd(sd.dhw_to_hwd(v), D)):
        assert bool((disp == -1).all())
        st = sd.lr_status(disp, disp, D)
        assert bool((st == 2).all())
        assert np.array_equal(st.cpu().numpy(), ref.lr_status(disp.cpu().numpy(), disp.cpu().numpy(), D))
        di = sd.interpolate(disp, st)
        assert bool((di == -1).all())
        assert bool((sd.subpixel(di, v) == -1).all()) and bool((sd.subpixel_hwd(di, sd.dhw_to_hwd(v), D) == -1).all())


# ---- a3: the explicit region list -------------------------------------------------------------------------------------
CANARY = 0x5A5A5A5A


@pytest.mark.parametrize("L", [14, 5])
@pytest.mark.parametrize("H,W", [(24, 32), (37, 61)])
def test_region_list_every_slot(H, W, L):
    """Every pixel's whole list, padding included, on an image with the longest arms (flat) and one with none (noise);
    support built and listed with the same L, (2L)^2 slots per pixel, canary words behind the buffer untouched."""
    import _hipabi as hip
    import oracle as o
    import stereo_device as sd
    lib = hip.load()
    rng = ref.case_rng(8, H, W, L)
    for name, img in (("flat", np.full((H, W), 0.25, dtype=np.float32)),
                      ("noise", rng.permutation(H * W).reshape(H, W).astype(np.float32))):     # no two pixels within tau
        support = sd.cross_arms(dev(img), 0.02, L)
        arms = sd.support_arms(support).cpu().numpy()
        assert np.array_equal(arms, o.cross_arms(img, 0.02, L)[0])                   # the arms the golden tests pin
        assert (arms.max() == L - 1) if name == "flat" else (arms.max() == 0)
        n = H * W * (2 * L) ** 2 * 2
        buf = torch.full((n + 256,), CANARY, dtype=torch.int32, device="cuda")
        rc = lib.mccnn_cross_region_list(hip.ptr(support), H, W, L, hip.ptr(buf), hip.stream())
        assert rc == 0, lib.mccnn_last_error_string()
        got = buf.cpu().numpy()
        assert (got[n:] == CANARY).all()
        want = ref.region_list(arms, L)
        assert np.array_equal(got[:n].reshape(want.shape), want), "%s %dx%d L=%d" % (name, H, W, L)
        assert np.array_equal((want[..., 0] >= 0).sum(-1), sd.support_count(support).cpu().numpy())


def test_region_list_refuses_a_plane_with_longer_arms():
    """A plane built at L = 14 has up to 27 * 27 entries per pixel; listed with L = 2 (16 slots) it would overrun its
    neighbours' slots and the buffer.  Refused like in the aggregation entry points; nothing is launched."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W = 24, 32
    support = sd.cross_arms(dev(np.full((H, W), 0.25, dtype=np.float32)), 0.02, 14)
    buf = torch.full((H * W * (2 * 14) ** 2 * 2,), CANARY, dtype=torch.int32, device="cuda")     # room for either L
    s = hip.stream()
    _rc(lib, lib.mccnn_cross_region_list(hip.ptr(support), H, W, 2, hip.ptr(buf), s), E_INVALID,
        b"mccnn_cross_region_list: support plane was built with distance 14, called with L=2")
    _rc(lib, lib.mccnn_cross_region_list(hip.ptr(support), H, W + 1, 14, hip.ptr(buf), s), E_INVALID,
        b"mccnn_cross_region_list: support plane was built for a 32x24 image")
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
