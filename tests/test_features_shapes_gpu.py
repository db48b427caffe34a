"""GPU: the matrix-core feature kernels (csrc/conv_mfma.hip) where a workgroup walks several tiles, on every route of
NET.features_pair_hwc_split, and one layer at a time through the C ABI.

conv3x3_split_kernel is persistent: one workgroup per compute unit walks 16 x 32 tiles in an XCD-contiguous order and
prefetches the next tile's first channel group under the last one of the current tile.  Up to 120 x 200 (the shapes
of test_features_split_gpu.py) no workgroup ever has a second tile.  Here:
  A. the whole stack against a float64 evaluation (helpers.features_float64, whole images or windows) at tile counts
     chosen from the device's compute units, ragged in both directions, and at the three benchmark sizes;
  B. the three routes of NET.features_pair_hwc_split (one batch of two / view by view / banded library convolutions)
     at the sizes where the kernels' 32-bit byte offsets are largest;
  C. bit-level invariances that need no reference: repeatability, independence of the other view and of the batch
     size, crop equivariance (a crop is a one-tile-per-workgroup run of the kind pinned to float64 elsewhere);
  D. one layer on hand-made records: exact routing of every channel, tap and pixel, arithmetic against float64, and
     the saturation flag of conv3x3_split - stored pixels only.
The bounds are the project's (tolerances.FEATURES_F32_CLASS_ABS, the split-vs-library rule of
test_split_features_as_close_to_float64_as_the_library_path).  Measured numbers go to the record file of
test_features_split_gpu.py, next to its keys; profiles/parity_features_shapes.json is a copy of them."""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tolerances as tol
from helpers import features_float64, records_decode, records_encode, smooth_pair, split_f16
from test_features_split_gpu import record_measured

pytestmark = pytest.mark.gpu

RECORD = {}
TRAINED = "converted reference checkpoint"


def _save():
    record_measured(RECORD)


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


@pytest.fixture(scope="module")
def cus8(sd):
    """The grid of the persistent kernel: compute units in whole groups of 8 (device_cus8 of csrc/abi_common.hip)."""
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count & ~7)


def _wide_range_net():
    """Weight magnitudes log-uniform over 2^-16 .. 1 of a layer's largest, biases of the size of the activations they
    meet (measured layer by layer in float64 on a small image)."""
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=11)
    g = torch.Generator().manual_seed(12)
    x = F.pad(smooth_pair(64, 64, 2)[0].double()[None, None], (5, 5, 5, 5))
    weights, biases = [], []
    for w in net.weights:
        w = w.cpu()
        w = (torch.sign(w) * float(w.abs().max()) * 2.0 ** (-16.0 * torch.rand(w.shape, generator=g))).float()
        y = F.conv2d(x, w.double())
        b = ((torch.rand((64,), generator=g) * 2 - 1) * 2.0 * float(y.pow(2).mean().sqrt())).float()
        x = F.relu(y + b.double()[None, :, None, None])
        weights.append(w.cuda())
        biases.append(b.cuda())
    net.weights, net.biases = weights, biases
    return net


@pytest.fixture(scope="module")
def nets(net_layers, sd):
    from model import NET
    trained = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    random_init = NET(None, input_patch_size=11, batch_size=1, device="cuda", seed=3)
    return {TRAINED: trained, "random init": random_init, "wide dynamic range": _wide_range_net()}


# ---- A. the whole stack against float64 where workgroups walk several tiles ----------------------------------------
def _tiles(H, W, n=2):
    return n * (-(-H // 16)) * (-(-W // 32))


def _shape(ty, tx, hr, wr):
    """ty x tx tiles with H % 16 == hr and W % 32 == wr."""
    return 16 * (ty - 1) + hr, 32 * (tx - 1) + wr


def _factor(n):
    a = math.isqrt(n)
    while n % a:
        a -= 1
    return a, n // a


def multi_tile_shapes(cus8):
    """{case: (H, W)} from the number of workgroups; T = 2 ceil(H / 16) ceil(W / 32) tiles in the last layer."""
    odd = math.isqrt(3 * cus8 // 2) | 1
    wide = odd
    while 2 * odd * wide <= 3 * cus8:
        wide += 2
    return {"one workgroup walks two tiles": _shape(*_factor(cus8 // 2 + 1), 1, 31),        # T = cus8 + 2 (T is even)
            "every workgroup walks two": _shape(*_factor(cus8), 15, 1),                       # T = 2 cus8
            "three or more and the xcd remainder": _shape(odd, wide, 1, 1),                   # T = 2 odd odd: T % 8 in {2, 6}
            "three or more, ragged 15 and 31": _shape(odd + 2, wide, 15, 31)}


def _windows(H, W, h=32, w=64):
    """Output windows (y0, y1, x0, x1) of a large image: the four corners, the last (partial) tile row and column, two
    interior tile seams (a multiple of 16 rows crossing a multiple of 32 columns), and the first and last rows away
    from the corners - the rows next to the other view in a batch of two."""
    def at(yc, xc):
        y0 = min(max(yc - h // 2, 0), H - h)
        x0 = min(max(xc - w // 2, 0), W - w)
        return (y0, y0 + h, x0, x0 + w)
    ly, lx = (H - 1) // 16 * 16, (W - 1) // 32 * 32          # where the last tile row / column begins
    sy, sx = H // 32 * 16, W // 64 * 32
    return sorted(set(at(*p) for p in ((0, 0), (0, W), (H, 0), (H, W), (ly, W // 2), (H // 2, lx), (ly, lx),
                                       (sy, sx), (sy + 48, sx + 160), (0, W // 2), (H, W // 2), (H, W // 3))))


def _errors(net, images, feats, windows):
    """max |feature - float64| over the views, on whole images (windows None) or on the windows."""
    e = 0.0
    for img, f in zip(images, feats):
        if windows is None:
            e = max(e, float((f.double().cpu() - features_float64(net, img)).abs().max()))
            continue
        for (y0, y1, x0, x1) in windows:
            ref = features_float64(net, img, (y0, y1, x0, x1))
            e = max(e, float((f[y0:y1, x0:x1].double().cpu() - ref).abs().max()))
    return e


def _both_paths_against_float64(nets, H, W, key, windows=None):
    bad = []
    for name, net in nets.items():
        L, R = smooth_pair(H, W, 7)
        lib = net.features_pair_hwc(L.cuda(), R.cuda())
        spl = net.features_pair_hwc_split(L.cuda(), R.cuda())
        assert spl[0].shape == (H, W, 64) and spl[0].dtype == torch.float32 and not net.split_saturated()
        e_lib, e_spl = _errors(net, (L, R), lib, windows), _errors(net, (L, R), spl, windows)
        RECORD["%s %dx%d %s" % (key, W, H, name)] = {"library_fp32_max_abs_err": e_lib, "split_f16_max_abs_err": e_spl,
                                                     "last_layer_tiles": _tiles(H, W),
                                                     "reference": "float64, whole images" if windows is None
                                                     else "float64, %d windows per view" % len(windows)}
        print("%s %dx%d %s: library %.3g split %.3g" % (key, W, H, name, e_lib, e_spl))
        if not e_spl <= tol.FEATURES_F32_CLASS_ABS:
            bad.append("%s: split path %g from float64" % (name, e_spl))
        if not e_lib <= tol.FEATURES_F32_CLASS_ABS:
            bad.append("%s: library path %g from float64" % (name, e_lib))
        if not e_spl <= 1.5 * e_lib + 5e-8:
            bad.append("%s: split %g vs library %g" % (name, e_spl, e_lib))
        del lib, spl
    _save()
    assert not bad, "%dx%d: %s" % (W, H, "; ".join(bad))


def test_the_chosen_shapes_walk_several_tiles_in_every_layer(cus8):
    s = multi_tile_shapes(cus8)
    t = {k: _tiles(*hw) for k, hw in s.items()}
    assert t["one workgroup walks two tiles"] == cus8 + 2
    assert t["every workgroup walks two"] == 2 * cus8
    for k in ("three or more and the xcd remainder", "three or more, ragged 15 and 31"):
        assert t[k] > 3 * cus8 and t[k] % 8 != 0, (k, t[k])
    assert {(H % 16, W % 32) for H, W in s.values()} == {(1, 31), (15, 1), (1, 1), (15, 31)}
    # the intermediate layers have H + 6, H + 4, H + 2 rows (and columns): their tile counts differ
    for grow in (6, 4, 2, 0):
        assert any(_tiles(H + grow, W + grow) > cus8 for H, W in s.values()), grow


@pytest.mark.parametrize("case", ["one workgroup walks two tiles", "every workgroup walks two",
                                  "three or more and the xcd remainder", "three or more, ragged 15 and 31"])
def test_whole_stack_against_float64_beyond_one_tile_per_workgroup(nets, cus8, case):
    H, W = multi_tile_shapes(cus8)[case]
    _both_paths_against_float64(nets, H, W, case)


@pytest.mark.parametrize("H,W", [(500, 750), (375, 1242)])
def test_whole_stack_against_float64_at_benchmark_size(nets, cus8, H, W):
    assert _tiles(H, W) > 3 * cus8
    _both_paths_against_float64(nets, H, W, "benchmark size")


def test_whole_stack_against_float64_windows_at_1500x1000(nets, cus8):
    H, W = 1000, 1500
    _both_paths_against_float64(nets, H, W, "benchmark size", _windows(H, W))


# ---- B. the three routes of NET.features_pair_hwc_split -------------------------------------------------------------
def _route_against_float64(net, key, H, W, route, windows):
    from model import split_feature_route
    got_route, rows = split_feature_route(H, W, 5)
    assert got_route == route
    L, R = smooth_pair(H, W, 9)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        feats = net.features_pair_hwc_split(L.cuda(), R.cuda())
    warned = any("library convolutions in bands" in str(w.message) for w in seen)
    assert warned == (route == "library")
    assert feats[0].shape == (H, W, 64) and not net.split_saturated()
    if rows is not None:                                         # windows across the band seams at rows k * rows
        assert rows < H
        windows = list(windows) + [(k - 16, k + 16, x0, x0 + 64) for k in range(rows, H - 16, rows)
                                   for x0 in (0, W // 2, W - 64)]
    e = _errors(net, (L, R), feats, windows)
    RECORD["route %s %dx%d %s" % (route, W, H, key)] = {
        "max_abs_err": e, "reference": "float64, %d windows per view" % len(windows),
        "records_of_limit": 2 * (H + 8) * (W + 8) / float(0x7ffffff0 // 256)}
    print("route %s %dx%d: %.3g" % (route, W, H, e))
    _save()
    del feats
    torch.cuda.empty_cache()
    assert e <= tol.FEATURES_F32_CLASS_ABS, "%s %dx%d: %g from float64" % (route, W, H, e)


def test_route_view_by_view_2100x2048(nets):
    for name in (TRAINED, "wide dynamic range"):
        _route_against_float64(nets[name], name, 2048, 2100, "views", _windows(2048, 2100))


def test_routes_with_byte_offsets_at_the_top_of_31_bits(nets):
    """One batch of two and one view alone, each within 1 % below the 2^31 - 16 bytes of records the kernels address:
    the load and store offsets of the last rows and columns use all their 31 bits."""
    limit = 0x7ffffff0 // 256
    H, W = 2037, 2043
    assert 0.99 * limit <= 2 * (H + 8) * (W + 8) <= limit
    _route_against_float64(nets[TRAINED], "pair at the limit", H, W, "pair", _windows(H, W))
    H, W = 2885, 2891
    assert 0.99 * limit <= (H + 8) * (W + 8) <= limit
    _route_against_float64(nets[TRAINED], "view at the limit", H, W, "views", _windows(H, W))


def test_route_library_bands_2900x2900(nets):
    _route_against_float64(nets[TRAINED], "bands", 2900, 2900, "library", _windows(2900, 2900))


def test_route_pair_whose_masked_rows_would_pass_2_31(nets):
    """2187 x 1900: in layer 2 (N = 2, Ho = 1906, Wo = 2193) the rows 1906 .. 1919 of the ragged last tile row of the
    right view would have the store offset ((n Ho + row) Wo + tx0) 256 >= 2^31 in the last tile columns; the kernel
    forms it from the last real row."""
    H, W = 1900, 2187
    Ho, Wo = H + 6, W + 6
    last_row, last_tx0 = 16 * (-(-Ho // 16)) - 1, (Wo - 1) // 32 * 32
    assert ((Ho + last_row) * Wo + last_tx0) * 256 >= 2 ** 31 > 2 * (H + 8) * (W + 8) * 256
    _route_against_float64(nets[TRAINED], "masked rows past 2^31", H, W, "pair", _windows(H, W))


# ---- C. bit-level invariances ------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("H,W", [(500, 750), (2048, 2100)])
def test_bit_level_invariances(nets, sd, H, W):
    """The sum of one output pixel has a fixed order (channel groups, taps, the matrix core's 16-channel step) that does
    not depend on the pixel's place in a tile, on the tile's place in a workgroup's walk, on the batch or on the other
    view - so these hold as uint32 patterns."""
    net = nets[TRAINED]
    L, R = smooth_pair(H, W, 13)
    l, r, r2 = L.cuda(), R.cuda(), smooth_pair(H, W, 14)[1].cuda()
    a = net.features_pair_hwc_split(l, r)
    b = net.features_pair_hwc_split(l, r)
    assert _same(a[0], b[0]) and _same(a[1], b[1]), "two runs on the same pair differ"
    del b
    assert _same(a[0], net.features_pair_hwc_split(l, r2)[0]), "the left features depend on the right view"
    x = sd.conv1_split(l[None].contiguous(), net.weights[0].detach().contiguous(), net.biases[0].detach(), 5)
    for k, (pk, ws) in enumerate(net._split_weights(), start=1):
        x = sd.conv3x3_split(x, pk, ws, net.biases[k].detach(), last=(k == net.num_conv_layers - 1))
    assert _same(a[0], x[0]), "the left features depend on the batch size"
    del x
    ch, cw = 96, 160
    for y0, x0 in ((3, 5), (H // 2 - 41, W // 2 + 7), (H - ch - 9, 1), (1, W - cw - 13), (H - ch, W - cw)):
        crop = l[y0:y0 + ch, x0:x0 + cw].contiguous()
        fc = net.features_pair_hwc_split(crop, crop)[0]
        assert _same(fc[5:-5, 5:-5], a[0][y0 + 5:y0 + ch - 5, x0 + 5:x0 + cw - 5]), \
            "crop at (%d, %d) differs from the whole image" % (y0, x0)
    assert not net.split_saturated()
    del a
    torch.cuda.empty_cache()


# ---- D. one layer at a time, through the C ABI, on hand-made records -----------------------------------------------------
def _layer_shape(cus8):
    """[N, Hi, Wi] with 17 tile rows (Ho % 16 = 1), Wo % 32 = 5 and more than two tiles per workgroup."""
    tx = cus8 // 17 + 1
    return 2, 16 * 16 + 1 + 2, 32 * (tx - 1) + 5 + 2


def _launch(sd, rec, w, b, last=False, flag=None):
    pk, ws = sd.conv3x3_split_pack(torch.from_numpy(w).cuda())
    return sd.conv3x3_split(rec, pk, ws, torch.from_numpy(b).cuda(), last=last, sat_flag=flag)


@pytest.mark.parametrize("tiny", [False, True])
def test_layer_routes_every_channel_tap_and_pixel_exactly(sd, cus8, tiny):
    """Weights W[o, pi(o), tap] = 1 for a permutation pi, everything else 0: out[o](y, x) = in[pi(o)](y + dy, x + dx)
    EXACTLY (the weight packs to hi = 1024, lo = 0, so an output is one exact product plus zeros and hi + lo fits
    float32).  Pins the lane maps of the pack kernel and the B fragments, the accumulator layout, halo, seams and the
    next-tile prefetch without a tolerance.  Second pass with a bias: relu(float32(256 v + 256 b)), one rounding (the
    kernel's single fmaf), split by the record rule."""
    S = sd.SPLIT_ACT_SCALE
    N, Hi, Wi = (2, 3, 3) if tiny else _layer_shape(cus8)
    Ho, Wo = Hi - 2, Wi - 2
    assert tiny or _tiles(Ho, Wo, N) > 2 * cus8
    rng = np.random.default_rng(5)
    rec = records_encode(rng.uniform(0, 4, (N, Hi, Wi, 64)).astype(np.float32), S)
    xin = records_decode(rec, S)
    assert (rec.view(np.float16).reshape(N, Hi, Wi, 4, 2, 16)[..., 1, :] != 0).mean() > 0.9
    d_rec = torch.from_numpy(rec).cuda()
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    pi = rng.permutation(64)
    bias = (rng.integers(-2048, 2048, 64) / 1024.0).astype(np.float32)        # 256 b + 256 v is exact in float64
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        w = np.zeros((64, 64, 3, 3), np.float32)
        w[np.arange(64), pi, dy, dx] = 1.0
        src = xin[:, dy:dy + Ho, dx:dx + Wo, :][..., pi]
        for b in (np.zeros(64, np.float32), bias):
            got = records_decode(_launch(sd, d_rec, w, b, flag=flag).cpu().numpy(), S)
            t = (src.astype(np.float64) * S + b.astype(np.float64) * S).astype(np.float32)
            hi, lo = split_f16(np.clip(t, 0.0, 65504.0))
            want = (hi.astype(np.float32) + lo.astype(np.float32)) / np.float32(S)
            if not b.any():
                assert np.array_equal(want, src)
            assert got.shape == want.shape
            wrong = got != want
            assert not wrong.any(), "tap %d%s: %d of %d values differ, first at %s" % (
                tap, " with bias" if b.any() else "", int(wrong.sum()), wrong.size, np.argwhere(wrong)[0])
    assert int(flag.item()) == 0


@pytest.mark.parametrize("last", [0, 1])
def test_layer_arithmetic_against_float64(sd, cus8, last):
    """Dense random weights on random records against a float64 convolution of the DECODED operands.  last=1 (unit
    vectors): the class bound.  last=0: relative to the layer's largest output, within 1.5 x the error of a float32
    evaluation of the same operands (the project's split-vs-library rule) plus 2^-22 for the records' quantisation."""
    from model import NET
    S = sd.SPLIT_ACT_SCALE
    N, Hi, Wi = _layer_shape(cus8)
    rng = np.random.default_rng(6)
    rec = records_encode(np.maximum(rng.standard_normal((N, Hi, Wi, 64)), 0).astype(np.float32) * 1.5, S)
    x = torch.from_numpy(records_decode(rec, S)).permute(0, 3, 1, 2).contiguous()
    net = NET(None, input_patch_size=11, batch_size=1, device="cpu", seed=3)
    w, b = net.weights[2], net.biases[2]
    out = _launch(sd, torch.from_numpy(rec).cuda(), w.numpy(), b.numpy(), last=bool(last)).cpu()
    ref = F.conv2d(x.double(), w.double(), b.double())
    if last:
        ref = ref / torch.sqrt(torch.clamp((ref * ref).sum(1, keepdim=True), min=1e-12))
        e = float((out.double().permute(0, 3, 1, 2) - ref).abs().max())
        RECORD["one layer last=1 %dx%dx%d" % (N, Wi, Hi)] = {"split_f16_max_abs_err": e}
        print("last=1: %.3g" % e)
        _save()
        assert e <= tol.FEATURES_F32_CLASS_ABS
        return
    ref = F.relu(ref)
    top = float(ref.abs().max())
    got = torch.from_numpy(records_decode(out.numpy(), S)).permute(0, 3, 1, 2)
    e = float((got.double() - ref).abs().max()) / top
    e32 = float((F.relu(F.conv2d(x, w, b)).double() - ref).abs().max()) / top
    RECORD["one layer last=0 %dx%dx%d" % (N, Wi, Hi)] = {"split_f16_max_err_rel_to_largest_output": e,
                                                         "float32_cpu_max_err_rel_to_largest_output": e32}
    print("last=0: kernel %.3g float32 %.3g" % (e, e32))
    _save()
    assert e <= 1.5 * e32 + 2.0 ** -22, "kernel %g, float32 evaluation %g" % (e, e32)


def test_saturation_flag_of_the_3x3_layer_counts_stored_pixels_only(sd):
    """conv3x3_split's own flag (the existing tests trip conv1_split's): inputs inside the records' range, outputs at,
    above and far below it, a NaN record, stickiness - and pixels of a ragged tile that are computed but never stored
    (columns >= Wo see the next row wrapped in, rows >= Ho the next view): they must not raise it."""
    S = sd.SPLIT_ACT_SCALE
    N, Hi, Wi = 2, 32 + 3 + 2, 32 + 7 + 2                        # Ho % 16 = 3, Wo % 32 = 7
    Ho, Wo = Hi - 2, Wi - 2
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    zero = np.zeros(64, np.float32)

    def run(x, w, b):
        rec = x if x.dtype == np.uint8 else records_encode(x, S)
        out = _launch(sd, torch.from_numpy(rec).cuda(), w, b, flag=flag)
        return records_decode(out.cpu().numpy(), S), int(flag.item())
    rng = np.random.default_rng(7)
    w = np.zeros((64, 64, 3, 3), np.float32)
    w[np.arange(64), np.arange(64), 1, 1] = 2.0                  # out[o](y, x) = 2 in[o](y + 1, x + 1)
    x = rng.uniform(0, 100, (N, Hi, Wi, 64)).astype(np.float32)
    x[1, 7, 9, 3] = 127.5
    base, f = run(x, w, zero)
    assert f == 0 and base.max() == 255.0 and base[1, 6, 8, 3] == 255.0
    neg = zero.copy()
    neg[5] = -1e3                                                # a large negative pre-activation: ReLU, no flag
    got, f = run(x, w, neg)
    assert f == 0 and not got[..., 5].any() and np.array_equal(np.delete(got, 5, -1), np.delete(base, 5, -1))
    x2 = x.copy()
    x2[0, 20, 30, 40] = 150.0                                    # one output at 300
    got, f = run(x2, w, zero)
    assert f == 1 and got[0, 19, 29, 40] == np.float32(65504.0 / 256.0)
    got[0, 19, 29, 40] = base[0, 19, 29, 40]
    assert np.array_equal(got, base), "a clamped output changed its neighbours"
    got, f = run(x, w, zero)
    assert f == 1 and np.array_equal(got, base), "a launch that does not saturate cleared the flag"
    flag.zero_()
    rec = records_encode(x, S).copy()
    rec.view(np.float16).reshape(N, Hi, Wi, 4, 2, 16)[1, 12, 13, 2, 0, 4] = np.float16(np.nan)
    assert run(rec, w, zero)[1] == 1, "a NaN record did not raise the flag"
    flag.zero_()
    # masked pixels: 3 v w = 199.5 is the largest stored output, the dropped ones reach 6 v w = 399
    c, o, v, wv = 7, 21, 1.0, 66.5
    w = np.zeros((64, 64, 3, 3), np.float32)
    w[o, c] = wv
    x = np.zeros((N, Hi, Wi, 64), np.float32)
    x[:, :, 0, c] = v
    x[:, :, Wi - 1, c] = v                                       # column Wo of a row sees column Wi - 1 and the next row's 0
    got, f = run(x, w, zero)
    assert got.max() == 3 * v * wv and got[0, 5, Wo - 1, o] == 3 * v * wv
    assert f == 0, "a column that is not stored raised the saturation flag"
    x = np.zeros((N, Hi, Wi, 64), np.float32)
    x[0, Hi - 1, :, c] = v
    x[1, 0, :, c] = v                                            # row Ho of the left view sees the right view's top row
    got, f = run(x, w, zero)
    assert got.max() == 3 * v * wv and got[0, Ho - 1, 5, o] == 3 * v * wv and got[1, 0, 5, o] == 3 * v * wv
    assert f == 0, "a row that is not stored raised the saturation flag"
