"""GPU: the metric outputs of include/mccnn.h - mccnn_depth and mccnn_reproject_points - bit for bit against the NumPy
restatement (tests/reproject_reference.py), as uint32 patterns: special values, red zones and odd bases for the depth
plane; count, order, bytes, unwritten tails, reuse of the buffers and replay of a captured graph for the cloud; then
StereoMatcher(geometry=...) at the golden pair's shape, eagerly, captured and on two matchers in flight.

The compaction takes 1024 pixels per block and scans 1024 block counts per workgroup of its second launch, so the pixel
counts are 1, 63 .. 65 (a wave), 1023 .. 1025 (a block) and LEVEL = 1025 x 1030 = 1 055 750 pixels: 1032 blocks, the
smallest handy shape whose block counts do not fit one workgroup of the scan, so that the third launch's carry decides
the ranks of the last blocks."""
import numpy as np
import pytest
import torch

import reproject_reference as ref

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
ZONE = 64                                   # red zone, in elements
LEVEL = (1025, 1030)
MIDDLEBURY = (3997.684, 3990.25, 1176.728, 1011.728, 193.001)       # fx != fy; the baseline in mm
TINY = (1e-3, 2e-3, 0.5, 0.25, 1e-20)                               # fb = 1e-23: Z underflows for large d
GOLDEN = (40, 48, 16)
RULE = "lr,speckle:20:1"


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


@pytest.fixture(scope="module")
def net(net_layers):
    from model import NET
    return NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(t):
    return np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def same(a, b, what):
    a, b = words(a), words(b)
    assert a.shape == b.shape and np.array_equal(a, b), "%s: %d of %d words differ" % (
        what, int((a != b).sum()) if a.shape == b.shape else -1, a.size)


def poisoned(n, shape, skew):
    """(whole buffer, the window of n float32 inside it) filled with POISON: ZONE elements on both sides, the window
    `skew` elements further on (1: a base that is 4-byte and not 8-byte aligned)."""
    whole = torch.full((n + 2 * ZONE + skew,), int(POISON.view(np.int32)), dtype=torch.int32, device="cuda").view(torch.float32)
    window = whole[ZONE + skew:ZONE + skew + n].view(*shape)
    assert window.data_ptr() % 16 == (4 * skew) % 16 and window.is_contiguous()
    return whole, window


def zones_untouched(whole, n, skew, what):
    w = words(whole)
    assert (w[:ZONE + skew] == POISON).all() and (w[ZONE + skew + n:] == POISON).all(), what + ": a red zone was written"


def specials(doffs):
    """Every special value of the definitions, for this doffs."""
    d = np.float32(doffs)
    below = np.nextafter(-d, np.float32(-np.inf), dtype=np.float32)
    above = np.nextafter(-d, np.float32(np.inf), dtype=np.float32)       # doffs = 0: the smallest subnormal, den subnormal
    return np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -d, below, above, 1e-40, 3e38, -3e38, 1.0, 255.0], dtype=np.float32)


def depth_maps(H, W, doffs):
    """The maps of one shape: a ramp with the specials sprinkled over it - or, where the shape has no room, one map per
    special value."""
    sp = specials(doffs)
    n = H * W
    if n < 4 * sp.size:
        return [np.full((H, W), v, dtype=np.float32) for v in sp] + [ref.ramp(H, W)]
    m = ref.ramp(H, W).reshape(-1)
    m[(np.arange(sp.size) * 2654435761 % n).astype(np.int64)] = sp
    m[0], m[n - 1] = sp[0], sp[5]
    return [m.reshape(H, W)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (3, 257), (37, 130)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("doffs", [0.0, 12.5, -3.0])
def test_depth_bits_special_values_and_red_zones(sd, shape, doffs):
    H, W = shape
    for intrinsics in (MIDDLEBURY, TINY):
        calib = intrinsics + (doffs,)
        for k, m in enumerate(depth_maps(H, W, doffs)):
            _, src = poisoned(H * W, shape, 1)
            src.copy_(dev(m))
            whole, out = poisoned(H * W, shape, 1)
            assert sd.depth(src, calib, out=out) is out
            want = ref.depth(m, calib)
            same(out, want, "depth %s doffs=%g map %d" % (shape, doffs, k))
            zones_untouched(whole, H * W, 1, "depth %s" % (shape,))
            same(src, m, "the input")
    # what the definitions say of the special values, of the restatement itself
    sp = specials(doffs)
    never = np.array([[sp[0], sp[1], sp[2], sp[5], sp[6]]])         # NaN, +inf, -inf, -doffs, the value below it
    assert np.isposinf(ref.depth(never, MIDDLEBURY + (doffs,))).all()
    assert ref.points(never, MIDDLEBURY + (doffs,)).shape == (0, 4)
    assert ref.depth(np.full((1, 1), 3e38, np.float32), TINY + (doffs,))[0, 0] == 0.0, "Z underflows"


def masked(H, W, mask, seed=0):
    """A ramp whose dropped pixels hold +inf."""
    n = H * W
    keep = np.zeros(n, dtype=bool)
    if mask == "all":
        keep[:] = True
    elif mask == "first":
        keep[0] = True
    elif mask == "last":
        keep[-1] = True
    elif mask == "alternating":
        keep[::2] = True
    elif mask == "random":
        keep = np.random.default_rng(seed).random(n) < 0.5
    else:
        assert mask == "none"
    m = ref.ramp(H, W).reshape(-1).copy()
    m[~keep] = np.inf
    return m.reshape(H, W), int(keep.sum())


def cloud(sd, m, calib, max_depth=np.inf, buffers=None):
    """One call into poisoned buffers (or the ones handed in): (the whole record buffer's words [N,4], n, buffers)."""
    H, W = m.shape
    if buffers is None:
        whole, points = poisoned(H * W * 4, (H * W, 4), 0)
        n_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        buffers = (whole, points, n_out, sd.points_scratch(H, W, "cuda"))
    whole, points, n_out, scratch = buffers
    got = sd.reproject(dev(m), calib, max_depth, out=points, n_out=n_out, scratch=scratch)
    assert got[0] is points and got[1] is n_out
    return words(points), int(words(n_out)[0]), buffers


def check_cloud(sd, m, calib, what, max_depth=np.inf, count=None):
    H, W = m.shape
    want = ref.points(m, calib, max_depth)
    got, n, (whole, _p, _n, _s) = cloud(sd, m, calib, max_depth)
    assert n == want.shape[0], "%s: n_points %d, the restatement has %d" % (what, n, want.shape[0])
    if count is not None:
        assert n == count, what
    same(got[:n], want, what + ": the records")
    assert (got[n:] == POISON).all(), what + ": a record at or beyond n_points was written"
    zones_untouched(whole, H * W * 4, 0, what)
    return want


SHAPES = [(1, 1), (1, 63), (1, 64), (5, 13), (3, 341), (32, 32), (25, 41), LEVEL]      # 1, 63, 64, 65, 1023, 1024, 1025
MASKS = ("all", "none", "first", "last", "alternating", "random")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_points_count_order_bits_and_unwritten_tail(sd, shape):
    H, W = shape
    calib = MIDDLEBURY + (12.5,)
    for mask in MASKS:
        m, count = masked(H, W, mask, seed=H * W)
        check_cloud(sd, m, calib, "%dx%d %s" % (H, W, mask), count=count)


def test_points_special_values_and_max_depth(sd):
    H, W = 37, 130
    for doffs in (0.0, 12.5, -3.0):
        m = depth_maps(H, W, doffs)[0]
        for intrinsics in (MIDDLEBURY, TINY):
            calib = intrinsics + (doffs,)
            check_cloud(sd, m, calib, "specials doffs=%g" % doffs)
            z = ref.depth(m, calib)
            finite = np.sort(z[np.isfinite(z)])
            limit = float(finite[finite.size // 2])              # exactly a pixel's Z: that pixel stays
            want = check_cloud(sd, m, calib, "max_depth = a pixel's Z, doffs=%g" % doffs, max_depth=limit)
            assert (want[:, 2] == np.float32(limit)).any() and 0 < want.shape[0] < finite.size
            check_cloud(sd, m, calib, "max_depth below every Z", max_depth=-1.0, count=0)
    with pytest.raises(ValueError, match="NaN"):
        sd.reproject(dev(m), MIDDLEBURY, float("nan"))


def test_points_two_maps_into_the_same_buffers(sd):
    calib = MIDDLEBURY + (0.0,)
    for shape in ((25, 41), LEVEL):
        a, na = masked(*shape, "all")
        b, nb = masked(*shape, "random", seed=5)
        got, n, buffers = cloud(sd, a, calib)
        assert n == na
        for m, count in ((b, nb), (a, na), (masked(*shape, "none")[0], 0), (b, nb)):
            got, n, _ = cloud(sd, m, calib, buffers=buffers)
            assert n == count, "a stale count: %d for %d" % (n, count)
            same(got[:n], ref.points(m, calib), "the second map's records")


def test_points_and_depth_captured_once_replayed_on_two_maps(sd):
    H, W = 37, 130
    calib = MIDDLEBURY + (12.5,)
    maps = [masked(H, W, "random", seed=s)[0] for s in (1, 2)]
    static = dev(maps[0])
    _, points = poisoned(H * W * 4, (H * W, 4), 0)
    n_out = torch.zeros((1,), dtype=torch.int32, device="cuda")
    z = torch.empty((H, W), dtype=torch.float32, device="cuda")
    scratch = sd.points_scratch(H, W, "cuda")

    def launches():
        sd.depth(static, calib, out=z)
        sd.reproject(static, calib, 5e4, out=points, n_out=n_out, scratch=scratch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for k in (0, 1, 0):
        static.copy_(dev(maps[k]))
        graph.replay()
        want = ref.points(maps[k], calib, 5e4)
        n = int(words(n_out)[0])
        assert n == want.shape[0] and 0 < n < H * W
        same(words(points)[:n], want, "replay on map %d: the records" % k)
        same(z, ref.depth(maps[k], calib), "replay on map %d: the depth" % k)


# ---- the matcher -----------------------------------------------------------------------------------------------------
CALIB_A = MIDDLEBURY + (12.5,)
CALIB_B = (1733.74, 1733.74, 792.27, 541.89, 536.62, 0.0)


def golden_pair(golden_cases):
    g = dict(golden_cases)["ref_40x48x16_s0.npz"]
    return dev(g["left_u8"]), dev(g["right_u8"])


def check_result(res, want_fields, calib, max_depth, semi, what):
    """res: a PairResult of device tensors.  The map fields have the plain matcher's bits; the metric fields equal the
    restatement applied to the returned dense / sparse map."""
    for got, want, name in zip(res[:3], want_fields, ("map", "planes", "sparse")):
        assert (got is None) == (want is None)
        if want is not None:
            same(got, want, "%s: %s" % (what, name))
    dense = res.map.cpu().numpy()
    same(res.depth, ref.depth(dense, calib), what + ": the depth plane")
    source = res.sparse.cpu().numpy() if semi else dense
    want = ref.points(source, calib, max_depth)
    n = int(words(res.n_points)[0])
    assert n == want.shape[0] and 0 < n, "%s: n_points %d against %d" % (what, n, want.shape[0])
    same(words(res.points)[:n], want, what + ": the cloud")
    return n


@pytest.mark.parametrize("semi", [None, RULE], ids=["dense", "semi_dense"])
def test_matcher_geometry(sd, net, golden_cases, semi):
    from pair_result import PairResult
    H, W, D = GOLDEN
    lu, ru = golden_pair(golden_cases)
    plain = sd.StereoMatcher(net, semi_dense=semi)
    want = plain.result_of(plain.match_u8(lu, ru, D))
    geometry = dict(calib=CALIB_A, depth=True, points=True, max_depth=2e5)
    m = sd.StereoMatcher(net, semi_dense=semi, geometry=geometry)
    res = m.match_u8(lu, ru, D)
    assert len(res) == (5 if semi else 4)
    n_dense = check_result(m.result_of(res), want[:3], CALIB_A, 2e5, semi, "eager")
    if semi:
        assert n_dense < int(np.isfinite(ref.depth(want.map.cpu().numpy(), CALIB_A)).sum()), "the cloud is the sparse map's"
    # depth_out= / points_out=, and a new calibration as a launch argument
    dout = torch.full((H, W), -7.0, device="cuda")
    pout = torch.full((H * W, 4), -7.0, device="cuda")
    m.set_calibration(CALIB_B)
    res = m.result_of(m.match_u8(lu, ru, D, depth_out=dout, points_out=pout))
    assert res.depth is dout and res.points is pout
    n = check_result(res, want[:3], CALIB_B, 2e5, semi, "depth_out= / points_out= under another calibration")
    assert (words(pout)[n:] == words(np.float32(-7.0))).all(), "records beyond n_points were written"
    with pytest.raises(ValueError):
        m.match_u8(lu, ru, D, depth_out=torch.zeros((H, W + 1), device="cuda"))
    with pytest.raises(ValueError):
        m.match_u8(lu, ru, D, points_out=torch.zeros((H * W, 3), device="cuda"))
    # captured: one graph per calibration, replayed when the calibration comes back
    graphed = sd.StereoMatcher(net, semi_dense=semi, geometry=geometry)
    for calib in (CALIB_A, CALIB_B, CALIB_A):
        graphed.set_calibration(calib)
        res = graphed.result_of(graphed.match_graph_u8(lu, ru, D))
        check_result(res, want[:3], calib, 2e5, semi, "match_graph_u8 under %r" % (calib,))
    assert len(graphed._graphs) == 2
    # only one of the two outputs
    only = sd.StereoMatcher(net, semi_dense=semi, geometry=dict(calib=CALIB_A, depth=True))
    res = only.result_of(only.match_u8(lu, ru, D))
    assert res.points is None and res.n_points is None and "points" not in only._ws[(H, W, D)]
    same(res.depth, ref.depth(res.map.cpu().numpy(), CALIB_A), "depth alone")
    assert isinstance(res, PairResult)


def test_two_matchers_in_flight_and_both_views(sd, net, golden_cases):
    H, W, D = GOLDEN
    lu, ru = golden_pair(golden_cases)
    plain = sd.StereoMatcher(net, semi_dense=RULE)
    want = plain.result_of(plain.match_u8(lu, ru, D))
    geometry = dict(calib=CALIB_A, depth=True, points=True)
    matchers = [sd.StereoMatcher(net, semi_dense=RULE, geometry=geometry, on_saturation="ignore") for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in matchers]
    results = []
    for m, s, calib in zip(matchers, streams, (CALIB_A, CALIB_B)):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.set_calibration(calib)
            results.append(m.result_of(m.match_u8(lu, ru, D)))
    torch.cuda.synchronize()
    for res, calib in zip(results, (CALIB_A, CALIB_B)):
        check_result(res, want[:3], calib, np.inf, True, "two in flight, %r" % (calib,))
    # views="both": the leading axis stays on the map fields, the metric fields are the left view's
    both_plain = sd.StereoMatcher(net, views="both", semi_dense=RULE)
    both_want = both_plain.result_of(both_plain.match_u8(lu, ru, D))
    both = sd.StereoMatcher(net, views="both", semi_dense=RULE, geometry=geometry)
    res = both.result_of(both.match_u8(lu, ru, D))
    same(res.map, both_want.map, "both views: the maps")
    same(res.sparse, both_want.sparse, "both views: the sparse maps")
    assert tuple(res.depth.shape) == (H, W) and tuple(res.points.shape) == (H * W, 4)
    left = res.view(0, True)
    check_result(left, (want.map, None, want.sparse), CALIB_A, np.inf, True, "both views: the left view's metric fields")
    assert res.view(1, True).depth is None and res.view(1, True).points is None


def test_workspace_grows_only_with_the_option(sd, net):
    import _hipabi
    H, W, D = GOLDEN
    scratch = int(_hipabi.load().mccnn_points_scratch_bytes(H, W))
    assert scratch == 16 and int(_hipabi.load().mccnn_points_scratch_bytes(*LEVEL)) == (1032 + 2) * 4 + 8
    base = sd.workspace_bytes(H, W, D)
    assert sd.workspace_bytes(H, W, D, depth=False, points=False) == base
    assert sd.workspace_bytes(H, W, D, depth=True) == base + H * W * 4
    assert sd.workspace_bytes(H, W, D, points=True) == base + H * W * 16 + scratch + 4
    m = sd.StereoMatcher(net, geometry=dict(calib=CALIB_A, depth=True, points=True))
    ws = m.workspace(H, W, D)
    held = sum(ws[k].numel() * ws[k].element_size() for k in ("depth", "points", "n_points", "points_scratch"))
    assert held == H * W * 20 + scratch + 4
    plain = sd.StereoMatcher(net)
    assert plain.geometry is None and not set(plain.workspace(H, W, D)) & {"depth", "points", "n_points", "points_scratch"}


def test_process_functional(sd):
    import process_functional as pf
    assert "depth_from_disparity" in pf.__all__ and "reproject" in pf.__all__
    m = depth_maps(37, 130, 12.5)[0]
    calib = MIDDLEBURY + (12.5,)
    same(pf.depth_from_disparity(m, calib), ref.depth(m, calib), "pf.depth_from_disparity")
    got = pf.reproject(m, ",".join(repr(v) for v in calib), 1e5)
    want = ref.points(m, calib, 1e5)
    assert got.shape == want.shape and got.dtype == np.float32
    same(got, want, "pf.reproject")
    assert torch.is_tensor(pf.reproject(dev(m), calib))
