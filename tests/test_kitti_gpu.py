"""GPU: the KITTI entry points (csrc/kitti.hip) against their NumPy restatements (tests/kitti_reference.py): every pixel of
the encode and of the background interpolation as bit patterns, the scorer's counts as integers and its four sums as
uint64 bit patterns, on the shapes where a wave, a segment or a chunk seam can go wrong."""
import numpy as np
import pytest

import evaluation_reference as ref
import kitti_reference as kr

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(result, n_thr):
    import evaluation as ev
    return ev.Metrics.from_result(result.cpu(), (0.0,) * n_thr).raw


def _check(got, want):
    for name in ref.REGIONS:
        g, w = got[name], want[name]
        assert (g["n_valid"], g["n_invalid"], g["n_bad"]) == (w["n_valid"], w["n_invalid"], w["n_bad"]), (name, g, w)
        for key in ("sum_abs", "sum_sq"):
            assert ref.bits(g[key]) == ref.bits(w[key]), (name, key, g[key], w[key])


# ---- encode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (3, 65), (7, 1025)], ids=lambda v: str(v))
def test_encode_equals_the_restatement(H, W):
    import stereo_device as sd
    rng = np.random.default_rng(100 * H + W)
    specials = kr.encode_specials()
    disp = rng.uniform(0, 260, (H, W)).astype(np.float32)
    ties = (rng.integers(0, 65536, (H, W)).astype(np.float32) + np.float32(0.5)) / np.float32(256)   # exact .5 codes
    disp = np.where(rng.random((H, W)) < 0.3, ties, disp).astype(np.float32)
    flat = disp.reshape(-1)
    want_special = {}
    for k, (v, code) in enumerate(specials):
        if k < flat.size:
            i = (k * 61) % flat.size if flat.size > len(specials) * 61 else k
            flat[i] = v
            want_special[i] = code
    if H * W == 1:
        flat[0] = np.float32(2.5 / 256)
        want_special = {0: 2}
    got = sd.kitti_encode_u16(_dev(disp)).cpu().numpy()
    assert got.dtype == np.uint16 and got.shape == (H, W)
    assert np.array_equal(got, kr.encode(disp))
    for i, code in want_special.items():
        assert got.reshape(-1)[i] == code, (i, flat[i], code)


def test_encode_decode_round_trip_is_within_half_a_code():
    import stereo_device as sd
    disp = np.random.default_rng(3).uniform(1.0 / 512, 255.9, (5, 333)).astype(np.float32)
    back = kr.decode(sd.kitti_encode_u16(_dev(disp)).cpu().numpy())
    assert np.abs(back.astype(np.float64) - disp.astype(np.float64)).max() <= 0.5 / 256


@pytest.mark.parametrize("H,W", [(1, 1), (3, 65), (7, 1025), (256, 256)], ids=lambda v: str(v))
def test_decode_equals_the_restatement(H, W):
    """(256, 256): every code once."""
    import stereo_device as sd
    code = np.random.default_rng(H + W).integers(0, 65536, (H, W)).astype(np.uint16)
    if H * W == 65536:
        code = np.arange(65536, dtype=np.uint16).reshape(H, W)
    else:
        code.reshape(-1)[::7] = 0
    got = sd.kitti_decode_u16(_dev(code)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(kr.u32(got), kr.u32(kr.decode(code)))
    assert np.array_equal(np.isposinf(got), code == 0)
    assert np.array_equal(sd.kitti_encode_u16(_dev(got)).cpu().numpy(), code)       # the encode is its inverse


# ---- background interpolation -----------------------------------------------------------------------------------------
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025, 2049)
HEIGHTS = (1, 2, 3, 65)


@pytest.fixture(scope="module")
def hole_maps():
    """Every (H, W) of the issue with its restated result, computed once."""
    out = {}
    for H in HEIGHTS:
        for W in WIDTHS:
            whole = {1: (), 2: (), 3: (), 65: (0, 1, 30, 31, 64)}[H]
            m = kr.make_holes_map(H, W, seed=10000 * H + W, whole_rows=whole)
            out[H, W] = (m, kr.interpolate_background_walk(m))
    return out


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", HEIGHTS)
def test_interpolation_equals_the_kits_walk(hole_maps, H, W):
    import stereo_device as sd
    m, want = hole_maps[H, W]
    assert (~kr.valid(m)).any() or W == 1
    src = _dev(m)
    got = sd.kitti_interpolate_background(src).cpu().numpy()
    assert np.array_equal(kr.u32(got), kr.u32(want))
    assert np.array_equal(kr.u32(src.cpu().numpy()), kr.u32(m))                   # the input is only read
    if W == 2049:
        assert (~kr.valid(m[0, 300:1600])).all() and kr.valid(got[0, 300:1600]).all()


@pytest.mark.parametrize("rows", [(0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)],
                         ids=["top", "middle", "bottom", "top2", "bottom2", "top_bottom", "all"])
def test_interpolation_with_whole_rows_invalid(rows):
    import stereo_device as sd
    m = kr.make_holes_map(3, 257, seed=77, whole_rows=rows)
    want = kr.interpolate_background_walk(m)
    got = sd.kitti_interpolate_background(_dev(m)).cpu().numpy()
    assert np.array_equal(kr.u32(got), kr.u32(want))
    if rows == (1,):
        assert not kr.valid(got[1]).any()             # a whole invalid row between valid ones stays, as in the kit
    if rows == (0, 1, 2):
        assert np.array_equal(kr.u32(got), kr.u32(m))


def test_interpolation_ties_and_signed_zeros():
    import stereo_device as sd
    nan = np.nan
    m = np.array([[2.0, nan, 2.0, -1.0, 1.0, np.inf, 3.0, 0.0, nan, -0.0, -0.0, nan, 0.0, nan, nan]], np.float32)
    want = kr.interpolate_background_walk(m)
    assert np.array_equal(kr.u32(want), kr.u32(kr.interpolate_background_nearest(m)))
    # equal neighbours and +-0.0: the left one; -0.0 against +0.0 compares equal, so again the left one
    assert np.array_equal(kr.u32(want[0, [1, 3, 5, 8, 11]]), kr.u32(np.array([2.0, 1.0, 1.0, 0.0, -0.0], np.float32)))
    got = sd.kitti_interpolate_background(_dev(m)).cpu().numpy()
    assert np.array_equal(kr.u32(got), kr.u32(want))


# ---- the scorer -------------------------------------------------------------------------------------------------------
SCORE_SHAPES = [(1, 1), (5, 1023), (3, 1025), (33, 2049)]


@pytest.fixture(scope="module")
def score_cases():
    return {s: kr.make_score_case(s[0], s[1], seed=1000 * s[0] + s[1]) for s in SCORE_SHAPES}


@pytest.mark.parametrize("interpolate", [False, True], ids=["plain", "interpolate"])
@pytest.mark.parametrize("with_noc", [True, False], ids=["noc", "no_noc"])
@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_scorer_equals_the_restatement(score_cases, shape, with_noc, interpolate):
    import stereo_device as sd
    disp, occ, noc = score_cases[shape]
    noc = noc if with_noc else None
    src = _dev(disp)
    out = sd.evaluate_kitti(src, _dev(occ), _dev(noc), kr.D1, interpolate=interpolate)
    assert out.numel() * out.element_size() == 192
    want = kr.evaluate(disp, occ, noc, kr.D1, interpolate=interpolate)
    _check(_raw(out, 1), want)
    assert np.array_equal(kr.u32(src.cpu().numpy()), kr.u32(disp))               # disp itself is never written
    if shape[0] * shape[1] >= 16 and not interpolate:
        assert (occ == 0).any() and want["all"]["n_invalid"] >= 4 and want["all"]["n_bad"][0] > 0


def test_d1_is_strict_on_both_bounds():
    """The placed pixels of make_score_case alone: of |err| = 3, 3+, 3, 3+ (g = 50), 5, 5+, 5- (g = 100, 0.05 g = 5) and
    4, 4+, 4- (g = 80, 0.05 g = 4) exactly the 3+ and the 5+ / 4+ ones are bad."""
    import stereo_device as sd
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    down = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    g = np.array([[50, 50, 50, 50, 100, 100, 100, 80, 80, 80]], np.float32)
    d = np.array([[53.0, up(53.0), 47.0, down(47.0), 105.0, up(105.0), down(105.0), 76.0, down(76.0), up(76.0)]], np.float32)
    occ = (g * 256).astype(np.uint16)
    assert np.float32(0.05) * np.float32(100) == np.float32(5) and np.float32(0.05) * np.float32(80) == np.float32(4)
    for k in range(10):
        one = sd.evaluate_kitti(_dev(d[:, k:k + 1]), _dev(occ[:, k:k + 1]), None, kr.D1)
        assert _raw(one, 1)["all"]["n_bad"] == [1 if k in (1, 3, 5, 8) else 0], k
    _check(_raw(sd.evaluate_kitti(_dev(d), _dev(occ), None, kr.D1), 1), kr.evaluate(d, occ, None, kr.D1))


def test_eight_thresholds_and_the_unused_counts():
    import evaluation as ev
    import stereo_device as sd
    import torch
    disp, occ, noc = kr.make_score_case(5, 1023, seed=9)
    for thr in (kr.D1, kr.THR8):
        out = torch.full((24,), -1, dtype=torch.int64, device="cuda")
        sd.evaluate_kitti(_dev(disp), _dev(occ), _dev(noc), thr, out=out)
        _check(_raw(out, len(thr)), kr.evaluate(disp, occ, noc, thr))
        full = ev.Metrics.from_result(out.cpu(), (0,) * 8).raw
        for name in ref.REGIONS:
            assert full[name]["n_bad"][len(thr):] == [0] * (8 - len(thr))


@pytest.mark.parametrize("interpolate", [False, True], ids=["plain", "interpolate"])
def test_accumulate_three_maps(interpolate):
    import stereo_device as sd
    total = sd.evaluate_result("cuda")
    want = None
    for k, (H, W) in enumerate([(5, 1023), (3, 1025), (9, 700)]):
        disp, occ, noc = kr.make_score_case(H, W, seed=40 + k)
        noc = noc if k != 1 else None
        sd.evaluate_kitti(_dev(disp), _dev(occ), _dev(noc), kr.THR8, interpolate=interpolate, out=total, accumulate=True)
        r = kr.evaluate(disp, occ, noc, kr.THR8, interpolate=interpolate)
        want = r if want is None else ref.accumulate(want, r)
    _check(_raw(total, 8), want)


@pytest.mark.parametrize("shape", [(5, 1023), (33, 2049)], ids=lambda s: "%dx%d" % s)
def test_without_relative_bounds_it_is_mccnn_evaluate(shape):
    """rel = 0, interpolate = 0: the 192 bytes of mccnn_evaluate on the decoded truth with mask = 255 * (gt_noc != 0)."""
    import datasets
    import stereo_device as sd
    disp, occ, noc = kr.make_score_case(shape[0], shape[1], seed=5, noc_follows_occ=True)
    assert np.array_equal(noc[noc != 0], occ[noc != 0]) and (noc != occ).any()
    thr = (0.5, 1.0, 2.0, 3.0)
    a = sd.evaluate_kitti(_dev(disp), _dev(occ), _dev(noc), tuple((t, 0.0) for t in thr)).cpu().numpy()
    gt = datasets.kitti_gt_to_float(occ)
    assert np.array_equal(kr.u32(gt), kr.u32(kr.decode(occ)))
    b = sd.evaluate(_dev(disp), _dev(gt), _dev((255 * (noc != 0)).astype(np.uint8)), thr).cpu().numpy()
    assert a.tobytes() == b.tobytes() and a.any()


def test_encode_and_score_captured_in_a_graph_and_replayed():
    import stereo_device as sd
    import torch
    H, W = 7, 293
    cases = [kr.make_score_case(H, W, seed=70 + k, holes=0.1) for k in range(3)]
    d, o, n = (_dev(a) for a in cases[0])
    out = sd.evaluate_result("cuda")
    code = torch.zeros((H, W), dtype=torch.uint16, device="cuda")
    scratch = sd.evaluate_kitti_scratch(H, W, "cuda", interpolate=True)
    sd.kitti_encode_u16(d, out=code)                                    # warm-up outside the capture
    sd.evaluate_kitti(d, o, n, kr.D1, interpolate=True, out=out, scratch=scratch)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sd.kitti_encode_u16(d, out=code)
        sd.evaluate_kitti(d, o, n, kr.D1, interpolate=True, out=out, scratch=scratch)
    for disp, occ, noc in cases[1:]:
        for dst, src in ((d, disp), (o, occ), (n, noc)):
            dst.copy_(_dev(src))
        graph.replay()
        torch.cuda.synchronize()
        eager = sd.evaluate_kitti(_dev(disp), _dev(occ), _dev(noc), kr.D1, interpolate=True)
        assert out.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
        _check(_raw(out, 1), kr.evaluate(disp, occ, noc, kr.D1, interpolate=True))
        assert np.array_equal(code.cpu().numpy(), sd.kitti_encode_u16(_dev(disp)).cpu().numpy())
        assert np.array_equal(code.cpu().numpy(), kr.encode(disp))


def test_wrappers_validate_their_arguments():
    import stereo_device as sd
    import torch
    d = torch.zeros((4, 5), device="cuda")
    g = torch.zeros((4, 5), dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError):
        sd.evaluate_kitti(d, torch.zeros((4, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        sd.evaluate_kitti(d, torch.zeros((4, 6), dtype=torch.uint16, device="cuda"))
    with pytest.raises(ValueError):
        sd.evaluate_kitti(d, g, thresholds=())
    with pytest.raises(ValueError):
        sd.evaluate_kitti(d, g, accumulate=True)
    with pytest.raises(sd.hip.MccnnHipError, match="negative"):
        sd.evaluate_kitti(d, g, thresholds=((3.0, -0.05),))
    with pytest.raises(sd.hip.MccnnHipError, match="out must not be disp"):
        sd.kitti_interpolate_background(d, out=d)
    with pytest.raises(ValueError):
        sd.kitti_encode_u16(d.double())
    with pytest.raises(sd.hip.MccnnHipError, match="scratch"):
        sd.evaluate_kitti(d, g, interpolate=True, scratch=sd.evaluate_kitti_scratch(4, 5, "cuda", interpolate=False))
