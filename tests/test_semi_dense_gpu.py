"""GPU: mccnn_speckle_filter and mccnn_semi_dense_select against the restatement of tests/semi_dense_reference.py.  Every
comparison is over the uint32 patterns of every pixel of `out` and of `sizes`, nothing left out.

Shapes: 1x1, 1x70, 70x1 (no vertical / no horizontal link), 3x65 (a row one pixel past the 64-pixel wave), 33x257 (a
row one pixel past the 256-thread workgroup, 9 workgroups of the counting launch), 96x130 (13 of them); the analytic maps
at 64x257 and 750x500; rows of 16385 pixels and 65536 rows, where the other post kernels change path."""
import ctypes

import numpy as np
import pytest
import torch

import semi_dense_reference as ref

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
CANARY_F = np.float32(-12345.0)
CANARY_U = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def run(disp, min_size, max_diff, scratch=None):
    """-> (out, sizes) as uint32 patterns."""
    import stereo_device as sd
    out, sizes = sd.speckle_filter(dev(disp), min_size, max_diff, want_sizes=True, scratch=scratch)
    return u32(out), u32(sizes)


def check(disp, max_diff, want_sizes, min_sizes, what):
    want_sizes = np.asarray(want_sizes, np.uint32)
    for min_size in min_sizes:
        want_out = ref.speckle_filter(disp, min_size, max_diff, sizes=want_sizes)[0]
        out, sizes = run(disp, min_size, max_diff)
        bad = np.flatnonzero(sizes.reshape(-1) != want_sizes.reshape(-1))
        assert bad.size == 0, "%s min_size %d: %d sizes differ, first at %d: got %d, want %d" % (
            what, min_size, bad.size, bad[0], sizes.reshape(-1)[bad[0]], want_sizes.reshape(-1)[bad[0]])
        assert np.array_equal(out, u32(want_out)), "%s min_size %d: out differs" % (what, min_size)
        assert np.isin(out, np.append(u32(disp)[ref.valid(disp)], u32(INF))).all()


RANDOM_SHAPES = [(1, 1), (1, 70), (70, 1), (3, 65), (33, 257), (96, 130)]
_RANDOM = {}


def random_case(shape, max_diff):
    """The map and its flood-filled sizes, computed once per (shape, max_diff)."""
    key = (shape, max_diff)
    if key not in _RANDOM:
        disp = ref.random_map(shape[0], shape[1], seed=shape[0] * 1000 + shape[1])
        _RANDOM[key] = (disp, ref.component_sizes(disp, max_diff))
    return _RANDOM[key]


@pytest.mark.parametrize("max_diff", [0.0, 1.0, float("inf")])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=["%dx%d" % s for s in RANDOM_SHAPES])
def test_random_maps_against_the_flood_fill(shape, max_diff):
    disp, want = random_case(shape, max_diff)
    if shape[0] * shape[1] >= 70:
        assert np.isnan(disp).any() and (disp == -1).any() and np.isinf(disp).any() and (want == 0).any()
    largest = int(want.max())
    check(disp, max_diff, want, sorted(set([1, 2, max(largest, 1), largest + 1])), "%dx%d max_diff %s" % (shape + (max_diff,)))


def test_exact_tie_links():
    one = np.float32(1.0)
    above = np.nextafter(one, np.float32(2))
    for a, b, max_diff, linked in ((0.0, 1.0, one, True), (0.0, 1.0, np.nextafter(one, np.float32(0)), False),
                                   (0.0, above, one, False), (3.0, 3.0, 0.0, True), (-0.0, 0.0, 0.0, True),
                                   (0.0, -0.0, 0.0, True), (0.5, 0.75, 0.25, True), (0.5, np.nextafter(np.float32(0.75), one), 0.25, False),
                                   (2.0, 2.0 + 2.0 ** -22, 0.0, False)):
        for disp in (np.array([[a, b]], np.float32), np.array([[a], [b]], np.float32), np.array([[b, a]], np.float32)):
            want = np.full(disp.shape, 2 if linked else 1, np.uint32)
            assert ref.linked(disp.reshape(-1)[0], disp.reshape(-1)[1], max_diff) == linked
            check(disp, max_diff, want, (1, 2), "tie %r %r max_diff %r" % (a, b, max_diff))


def test_transitive_ramp():
    for H, W in ((1, 300), (300, 1), (5, 130)):
        disp = np.arange(H * W, dtype=np.float32).reshape(H, W)
        if H > 1 and W > 1:                                    # a boustrophedon ramp: rows joined at alternating ends only
            disp[1::2] = disp[1::2, ::-1]
        check(disp, 1.0, np.full((H, W), H * W, np.uint32), (1, H * W, H * W + 1), "ramp %dx%d" % (H, W))
        check(disp, np.nextafter(np.float32(1), np.float32(0)), np.ones((H, W), np.uint32), (1, 2), "ramp below 1")


def serpentine(H, W):
    """Corridor rows of zeros between walls of -1; each wall has one gap, at alternating ends: one component whose label
    chains run the whole corridor.  -> (map, sizes)."""
    disp = np.zeros((H, W), np.float32)
    disp[1::2] = -1.0
    walls = np.arange(1, H, 2)
    disp[walls, np.where((walls // 2) % 2 == 0, W - 1, 0)] = 0.0
    size = ((H + 1) // 2) * W + H // 2
    return disp, np.where(disp == 0, size, 0).astype(np.uint32)


def comb(H, W):
    """Teeth on the even columns that meet only in the last row.  -> (map, sizes)."""
    disp = np.full((H, W), np.nan, np.float32)
    disp[:, ::2] = 7.0
    disp[H - 1] = 7.0
    size = ((W + 1) // 2) * (H - 1) + W
    return disp, np.where(disp == 7.0, size, 0).astype(np.uint32)


@pytest.mark.parametrize("shape", [(64, 257), (750, 500)], ids=["64x257", "750x500"])
def test_analytic_shapes(shape):
    H, W = shape
    n = H * W
    check(np.full((H, W), 3.5, np.float32), 0.0, np.full((H, W), n, np.uint32), (1, n, n + 1), "constant")
    rows = np.zeros((H, W), np.float32)
    rows[1::2] = 10.0
    check(rows, 1.0, np.full((H, W), W, np.uint32), (W, W + 1), "alternating rows")
    board = ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 * 10).astype(np.float32)
    check(board, 1.0, np.ones((H, W), np.uint32), (1, 2), "checkerboard")
    disp, want = serpentine(H, W)
    check(disp, 0.0, want, (int(want.max()), int(want.max()) + 1), "serpentine")
    disp, want = comb(H, W)
    check(disp, 0.0, want, (int(want.max()), int(want.max()) + 1), "comb")


def test_analytic_shapes_agree_with_the_flood_fill():
    """The closed forms above, checked once against the flood fill at a small size."""
    for make in (serpentine, comb):
        for H, W in ((7, 9), (8, 6)):
            disp, want = make(H, W)
            assert np.array_equal(ref.component_sizes(disp, 0.0), want), make.__name__


@pytest.mark.parametrize("shape", [(1, 16385), (2, 16385), (65536, 2)], ids=["1x16385", "2x16385", "65536x2"])
def test_special_row_shapes(shape):
    H, W = shape
    n = H * W
    check(np.zeros((H, W), np.float32), 0.0, np.full((H, W), n, np.uint32), (n, n + 1), "constant")
    disp = ref.random_map(H, W, seed=W, levels=2)
    want = ref.component_sizes_equal_values(disp)
    check(disp, 0.0, want, (1, 3, int(want.max())), "random")


def test_partial_outputs_repeats_and_replay():
    import stereo_device as sd
    H, W = 33, 257
    disp, want_sizes = random_case((H, W), 1.0)
    min_size = 5
    want_out = u32(ref.speckle_filter(disp, min_size, 1.0, sizes=want_sizes)[0])
    d = dev(disp)
    before = u32(d).copy()
    scratch = sd.speckle_scratch(H, W, "cuda")
    both = sd.speckle_filter(d, min_size, 1.0, want_sizes=True, scratch=scratch)
    only_out = sd.speckle_filter(d, min_size, 1.0, scratch=scratch)
    only_sizes = sd.speckle_filter(d, min_size, 1.0, want_out=False, want_sizes=True, scratch=scratch)
    assert only_out[1] is None and only_sizes[0] is None
    for out in (both[0], only_out[0]):
        assert np.array_equal(u32(out), want_out)
    for sizes in (both[1], only_sizes[1]):
        assert np.array_equal(u32(sizes), want_sizes)
    assert np.array_equal(u32(d), before), "the dense map was written"
    # another map on the same scratch, then the first again: nothing of an earlier call survives in the scratch
    other, other_sizes = random_case((H, W), 0.0)
    assert np.array_equal(u32(sd.speckle_filter(dev(other), 1, 0.0, want_sizes=True, scratch=scratch)[1]), other_sizes)
    again = sd.speckle_filter(d, min_size, 1.0, want_sizes=True, scratch=scratch)
    assert np.array_equal(u32(again[0]), want_out) and np.array_equal(u32(again[1]), want_sizes)
    # captured, then replayed three times on changing input
    out = torch.empty_like(d)
    sizes = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sd.speckle_filter(d, min_size, 1.0, out=out, sizes=sizes, scratch=scratch)
    for k in range(3):
        d.copy_(dev(other if k == 1 else disp))
        out.fill_(float(CANARY_F))
        sizes.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        if k == 1:
            assert np.array_equal(u32(sizes), ref.component_sizes(other, 1.0))
        else:
            assert np.array_equal(u32(out), want_out) and np.array_equal(u32(sizes), want_sizes), "replay %d" % k


def test_refused_calls_write_nothing():
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W = 6, 10
    d = dev(np.zeros((H, W), np.float32))
    out = torch.full((H, W), float(CANARY_F), device="cuda")
    sizes = torch.full((H, W), CANARY_U, dtype=torch.int32, device="cuda")
    scratch = sd.speckle_scratch(H, W, "cuda")
    nbytes = scratch.numel() * 4
    st = hip.stream()
    p = hip.ptr

    def call(disp=p(d), h=H, w=W, max_diff=1.0, min_size=1, o=p(out), s=p(sizes), sc=p(scratch), n=nbytes):
        return lib.mccnn_speckle_filter(disp, h, w, max_diff, min_size, o, s, sc, n, st)

    assert call(max_diff=float("nan")) == hip.MCCNN_E_INVALID
    assert call(max_diff=-1.0) == hip.MCCNN_E_INVALID
    assert call(min_size=0) == hip.MCCNN_E_INVALID
    assert call(o=None, s=None) == hip.MCCNN_E_INVALID
    assert call(o=p(d)) == hip.MCCNN_E_INVALID and b"overlaps" in lib.mccnn_last_error_string()
    assert call(s=p(out)) == hip.MCCNN_E_INVALID and b"overlaps" in lib.mccnn_last_error_string()
    assert call(sc=p(out)) == hip.MCCNN_E_INVALID
    assert call(n=nbytes - 1) == hip.MCCNN_E_SCRATCH
    assert call(sc=ctypes.c_void_p(scratch.data_ptr() + 4), n=nbytes + 64) == hip.MCCNN_E_SCRATCH
    assert call(h=0) == hip.MCCNN_E_INVALID
    sel = lib.mccnn_semi_dense_select
    mc = (ctypes.c_float * 4)(0, 0, 0, 0)
    assert sel(p(d), None, None, H, W, 0, 0, mc, 0, p(d), st) == hip.MCCNN_E_INVALID      # out overlaps disp
    assert sel(p(d), p(sizes), None, H, W, 0, 0, mc, 1, p(sizes), st) == hip.MCCNN_E_INVALID
    assert sel(p(d), None, p(out), H, W, 1, 1, mc, 0, p(out), st) == hip.MCCNN_E_INVALID
    assert sel(p(d), None, p(d), H, W, 1, 3, mc, 0, p(out), st) == hip.MCCNN_E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY_F).all() and (u32(sizes) == CANARY_U).all()
    assert call() == 0 and call(s=None) == 0 and call(o=None) == 0
    torch.cuda.synchronize()
    assert (u32(sizes) == H * W).all() and (out.cpu().numpy() == 0).all()


# ---- the selection alone -------------------------------------------------------------------------------------------------
def _planes():
    """The four planes of a 24x40x16 volume, as mccnn_confidence_hwd writes them, plus the disparity it belongs to."""
    import confidence_reference as cref
    import stereo_device as sd
    H, W, D = 24, 40, 16
    vol = cref.make_volume(H, W, D, "normal", seed=11)
    right = cref.make_right_map(vol, seed=12)
    planes = sd.confidence_hwd(dev(cref.to_hwd(vol, np.nan)), D, dev(right), cref.NAMES)
    _, d1 = cref.confidence(vol, right, 15)
    disp = d1.astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0], np.float32)
    disp.reshape(-1)[5::13] = odd[np.arange(len(disp.reshape(-1)[5::13])) % 5]
    return disp, planes.cpu().numpy()


def test_selection_every_subset():
    import stereo_device as sd
    disp, planes = _planes()
    H, W = disp.shape
    rng = np.random.default_rng(3)
    status = rng.choice(np.array([0, 0, 0, 1, 2, 7], np.int32), (H, W)).astype(np.int32)
    assert np.isnan(planes).any() and (planes == -np.inf).any()
    d, s = dev(disp), dev(status)
    for have in range(0, 16):
        names = tuple(n for n in ref.NAMES if have & ref.BITS[n])
        sub = np.stack([planes[ref.NAMES.index(n)] for n in names]) if names else None
        dsub = dev(sub) if names else None
        for use in range(0, 16):
            if use & ~have:
                continue
            for variant in ("value", "above", "low"):
                thr = {}
                for n in names:
                    if not use & ref.BITS[n]:
                        continue
                    finite = np.sort(planes[ref.NAMES.index(n)][np.isfinite(planes[ref.NAMES.index(n)])])
                    v = np.float32(finite[len(finite) // 2])
                    thr[n] = {"value": v, "above": np.nextafter(v, INF), "low": np.float32(-np.inf)}[variant]
                for require_match in (False, True):
                    want = ref.select(disp, status, sub, names, thr, require_match)
                    out = torch.full((H + 1, W), float(CANARY_F), device="cuda")
                    got = sd.semi_dense_select(d, s if require_match else None, dsub, names, thr, require_match, out=out[:H])
                    assert got.data_ptr() == out.data_ptr()
                    host = out.cpu().numpy()
                    assert np.array_equal(u32(host[:H]), u32(want)), (names, use, variant, require_match)
                    assert (host[H] == CANARY_F).all()
    # a threshold equal to a plane value keeps that pixel, the next float above drops it
    mmn = planes[1]
    h, w = np.argwhere(np.isfinite(mmn) & ref.valid(disp))[7]
    v = np.float32(mmn[h, w])
    kept = sd.semi_dense_select(d, None, dev(planes), ref.NAMES, {"mmn": v}).cpu().numpy()
    dropped = sd.semi_dense_select(d, None, dev(planes), ref.NAMES, {"mmn": np.nextafter(v, INF)}).cpu().numpy()
    assert u32(kept)[h, w] == u32(disp)[h, w] and dropped[h, w] == INF
    # -inf as a threshold keeps -inf planes and still drops NaN ones
    low = sd.semi_dense_select(d, None, dev(planes), ref.NAMES, {"mmn": float("-inf")}).cpu().numpy()
    assert np.array_equal(u32(low), u32(ref.select(disp, None, planes, ref.NAMES, {"mmn": -np.inf})))
    assert (low[np.isnan(mmn)] == INF).all()


def test_semi_dense_is_selection_then_speckle():
    import stereo_device as sd
    disp, planes = _planes()
    H, W = disp.shape
    status = (np.random.default_rng(4).random((H, W)) < 0.2).astype(np.int32)
    for text in ("lr,speckle:20:1", "lr", "speckle:3", "mmn:0.5,lr,speckle:4:0", "msm:-1e30,cur:0,lrc:-1"):
        rule = sd.SemiDenseRule.parse(text)
        want = ref.semi_dense(disp, rule, status, planes, ref.NAMES)
        sizes = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        got = sd.semi_dense(dev(disp), text, dev(status), dev(planes), ref.NAMES, sizes=sizes)
        assert np.array_equal(u32(got), u32(want)), text
        if rule.speckle:
            selected = ref.select(disp, status, planes, ref.NAMES, rule.thresholds, rule.require_match)
            assert np.array_equal(u32(sizes), ref.component_sizes(selected, rule.speckle[1])), text
