"""GPU: the three epilogues of the library feature path (csrc/post.hip: mccnn_bias_act, mccnn_conv1_pad_bias_relu,
mccnn_l2norm_chw_to_hwc) called directly, where the whole-stack feature tolerances cannot hide a wrong tail element,
an unaligned plane or a dropped NaN.

  * mccnn_bias_act is one float32 add and a ReLU: bit-exact against NumPy.
  * The ReLU of both kernels is `t <= 0 ? 0 : t`: NaN stays NaN (NumPy's, torch's and TensorFlow's ReLU; fmaxf(NaN, 0)
    would be 0), ReLU(-0.0) = +0.0, every other input as np.maximum(t, 0).
  * mccnn_conv1_pad_bias_relu and mccnn_l2norm_chw_to_hwc against float64, with bounds DERIVED from the arithmetic
    (written where they are used), not measured; the largest errors seen are printed and, when MCCNN_RECORD_DIR names
    a directory, written to parity_epilogues.json there: profiles/parity_epilogues.json is a copy of that file."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import _describe, assert_bits, bits_strict

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit roundoff of float32
CANARY = np.float32(-12345.5)
E_UNSUPPORTED = -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relu(t):
    """The documented ReLU of the epilogues: NaN propagates, -0.0 -> +0.0."""
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, np.float32(0), t).astype(t.dtype)


def record_measured(record):
    out = os.environ.get("MCCNN_RECORD_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "parity_epilogues.json")
        old = {}
        if os.path.isfile(path):
            with open(path) as f:
                old = json.load(f)
        old.update(record)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- mccnn_bias_act ---------------------------------------------------------------------------------------------------
def bias_act_case(N, C, plane, relu_on, front, rng, specials):
    import stereo_device as sd
    total = N * C * plane
    x = (rng.standard_normal(total) * 2).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    b[0] = np.float32(-0.0) if C > 1 else b[0]
    if C > 2:
        b[C - 1] = np.float32(1e-40)                                     # a subnormal bias
    x3 = x.reshape(N, C, plane)
    edge = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38], dtype=np.float32)
    for n in range(N):
        for c in range(C):
            k = int(rng.integers(plane))
            x3[n, c, k] = edge[(n * C + c) % len(edge)]
            x3[n, c, plane - 1] = edge[(n * C + c + 3) % len(edge)]      # the tail element of the plane
            if plane > 2:
                x3[n, c, int(rng.integers(plane))] = -b[c]               # x + b == 0 exactly
    for i, v in enumerate(specials):                                     # not to be overwritten by the edge values
        x[(5 * i) % total] = v
        x[total - 1 - i % total] = v
    buf = np.full(front + total + 64, CANARY, dtype=np.float32)
    buf[front:front + total] = x
    dbuf = dev(buf)
    view = dbuf[front:front + total].view(N, C, 1, plane)
    assert view.is_contiguous() and view.data_ptr() == dbuf.data_ptr() + 4 * front
    sd.bias_act_(view, dev(b), relu_on)
    got = dbuf.cpu().numpy()
    with np.errstate(invalid="ignore"):
        t = x3 + b[None, :, None]
        want = relu(t) if relu_on else t
        if relu_on:                                                      # NumPy's own ReLU: same values everywhere
            assert np.array_equal(want, np.maximum(t, np.float32(0)), equal_nan=True)
    assert (got[:front] == CANARY).all() and (got[front + total:] == CANARY).all(), "wrote outside the tensor"
    return got[front:front + total].reshape(N, C, plane), want


def test_bias_act_bit_exact():
    """Planes of 1 .. 5, 1023 .. 1025 and 35 * 41 elements (tails of the 4-wide accesses; odd planes put later planes at
    addresses that are only 4-byte aligned, and so does an odd offset of the tensor itself), C = 1, 3, 64, N = 1, 2,
    with and without ReLU, -0.0, subnormals and exact zeros of x + b; canary values around the tensor stay."""
    rng = np.random.default_rng(11)
    failures, total = [], 0
    for plane in (1, 2, 3, 4, 5, 1023, 1024, 1025, 35 * 41):
        for C in (1, 3, 64):
            for N in (1, 2):
                for relu_on in (False, True):
                    total += 1
                    front = 64 if total % 2 else 67
                    got, want = bias_act_case(N, C, plane, relu_on, front, rng, [])
                    if not bits_strict(got, want):
                        failures.append("N=%d C=%d plane=%d relu=%d front=%d: %s" % (N, C, plane, relu_on, front,
                                                                                    _describe(got, want)))
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), total, "\n".join(failures))


def test_bias_act_relu_propagates_nan():
    """fmaxf(NaN, 0) is 0; NumPy's, torch's and TensorFlow's ReLU return NaN.  +-inf behave as in np.maximum."""
    rng = np.random.default_rng(12)
    for plane in (1, 5, 1025):
        for relu_on in (False, True):
            got, want = bias_act_case(2, 3, plane, relu_on, 67, rng, [np.nan, np.inf, -np.inf])
            assert np.isnan(want).any()
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert_bits(got, want, "bias_act with NaN, plane %d relu %d" % (plane, relu_on))


def test_bias_act_refuses_more_planes_than_the_grid():
    import _hipabi as hip
    lib = hip.load()
    x = torch.full((1024 * 64,), 3.0, device="cuda")
    b = torch.ones((64,), device="cuda")
    rc = lib.mccnn_bias_act(hip.ptr(x), hip.ptr(b), 1024, 64, 1, 1, hip.stream())
    assert rc == E_UNSUPPORTED and b"N*C=65536" in lib.mccnn_last_error_string()
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())
    assert lib.mccnn_bias_act(hip.ptr(x), hip.ptr(b), 1023, 64, 1, 1, hip.stream()) == 0     # 65472 planes are served
    torch.cuda.synchronize()
    assert bool((x[:1023 * 64] == 4.0).all()) and bool((x[1023 * 64:] == 3.0).all())


# ---- mccnn_conv1_pad_bias_relu ------------------------------------------------------------------------------------------
def conv1_float64(img, w, b, pad):
    """-> (the pre-activation in float64, sum |w v| + |b| per output): zero padding, 3x3 VALID cross-correlation."""
    N, H, W = img.shape
    C = w.shape[0]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad), dtype=np.float64)
    xp[:, pad:pad + H, pad:pad + W] = img
    acc = np.zeros((N, C, Ho, Wo), dtype=np.float64)
    mag = np.zeros((N, C, Ho, Wo), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(3):
            for j in range(3):
                term = w[:, 0, i, j].astype(np.float64)[None, :, None, None] * xp[:, None, i:i + Ho, j:j + Wo]
                acc += term
                mag += np.abs(term)
    bb = b.astype(np.float64)[None, :, None, None]
    return acc + bb, mag + np.abs(bb)


CONV1_SHAPES = [(3, 3), (3, 4), (4, 5), (7, 300), (11, 257), (5, 256)]


def test_conv1_pad_bias_relu_against_float64():
    """Pads 0, 1, 5 (the real one), images from 3x3 (pad 0: a 1x1 output) to 7x300 (rows of two blocks), N = 2, C = 64
    and 5.  DERIVED bound: the kernel forms 9 products and adds them and the bias in float32, in whatever order and
    contraction the compiler chooses, so every term passes through at most 10 roundings:
        |err| <= gamma_10 * (sum |w v| + |b|),  gamma_10 = 10 u to first order, u = 2^-24,
    evaluated per output in float64.  The ReLU is 1-Lipschitz, so clamped outputs are compared after the clamp under the
    same bound.  A wrong tap, a shifted pad or a missing bias is orders of magnitude above it."""
    import stereo_device as sd
    rng = np.random.default_rng(13)
    worst = 0.0
    for C in (64, 5):
        for pad in (0, 1, 5):
            for H, W in CONV1_SHAPES:
                img = rng.standard_normal((2, H, W)).astype(np.float32)
                w = (rng.standard_normal((C, 1, 3, 3)) * 0.5).astype(np.float32)
                w[0, 0, 1, 1] = 0
                b = rng.standard_normal(C).astype(np.float32)
                got = sd.conv1_pad_bias_relu(dev(img), dev(w), dev(b), pad).cpu().numpy()
                pre, mag = conv1_float64(img, w, b, pad)
                assert got.shape == pre.shape == (2, C, H + 2 * pad - 2, W + 2 * pad - 2)
                err = np.abs(got.astype(np.float64) - np.maximum(pre, 0.0))
                bound = 10 * U * mag
                ratio = float((err / bound).max())
                print("conv1 C=%d pad=%d %dx%d: max |err| %.3g, max err / bound %.3g" % (C, pad, H, W, err.max(), ratio))
                worst = max(worst, ratio)
                assert (err <= bound).all(), "C=%d pad=%d %dx%d: |err| up to %g, %g of the derived bound" % (
                    C, pad, H, W, err.max(), ratio)
                assert (got >= 0).all() and (got == 0).any() and (got > 0).any()
    record_measured({"conv1_pad_bias_relu": {"bound": "10 * 2^-24 * (sum |w v| + |b|) per output",
                                             "largest_error_as_a_fraction_of_the_bound": worst}})


def test_conv1_nan_pixel_reaches_its_outputs_and_nothing_else():
    """A NaN input pixel gives NaN at every output whose 3x3 window holds it, in every map, and nowhere else."""
    import stereo_device as sd
    rng = np.random.default_rng(14)
    for pad, (H, W), (y, x) in ((5, (6, 9), (2, 4)), (1, (5, 7), (0, 0)), (0, (5, 300), (4, 256)), (5, (4, 5), (3, 4))):
        img = rng.standard_normal((2, H, W)).astype(np.float32)
        img[1, y, x] = np.nan
        w = (rng.standard_normal((5, 1, 3, 3)) * 0.5).astype(np.float32)
        w[2] = -np.abs(w[2])                                           # a map that would otherwise mostly clamp to 0
        b = rng.standard_normal(5).astype(np.float32)
        got = sd.conv1_pad_bias_relu(dev(img), dev(w), dev(b), pad).cpu().numpy()
        pre, mag = conv1_float64(img, w, b, pad)
        assert np.isnan(pre).sum() in (5 * 9, 5 * 4, 5 * 6, 5 * 3, 5 * 2, 5) and not np.isnan(pre[0]).any()
        assert np.array_equal(np.isnan(got), np.isnan(pre)), "pad %d %dx%d" % (pad, H, W)
        ok = ~np.isnan(pre)
        assert (np.abs(got.astype(np.float64) - np.maximum(pre, 0.0))[ok] <= (10 * U * mag)[ok]).all()


def test_nan_image_gives_nan_features_on_the_library_route(net_layers):
    """A constant image standardises to 0 / 0 = NaN everywhere; the split route raises its saturation flag for it and
    the pair is recomputed on the library route, which must hand back NaN like the reference - not the finite features
    of an all-zero image that an fmaxf ReLU produced."""
    import process_functional as pf
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    H, W = 12, 20
    nan_img = torch.full((H, W), float("nan"), device="cuda")
    f = net.features_hwc(nan_img)
    assert tuple(f.shape) == (H, W, 64) and bool(torch.isnan(f).all())
    const = np.full((H, W, 1), 7.0, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        std = (const - const.mean()) / const.std()
    assert np.isnan(std).all()
    fl, fr = pf.compute_features(std, std, 11, 11, net)
    assert np.isnan(fl).all() and np.isnan(fr).all()
    # one NaN pixel poisons the 11x11 outputs that see it and no other
    img = torch.from_numpy(np.random.default_rng(15).standard_normal((H + 8, W + 8)).astype(np.float32)).cuda()
    img[10, 14] = float("nan")
    bad = torch.isnan(net.features_hwc(img)).all(dim=-1).cpu().numpy()
    want = np.zeros((H + 8, W + 8), bool)
    want[5:16, 9:20] = True
    assert np.array_equal(bad, want)
    assert np.array_equal(torch.isnan(net.features_hwc(img)).any(dim=-1).cpu().numpy(), want)


# ---- mccnn_l2norm_chw_to_hwc ------------------------------------------------------------------------------------------
def test_l2norm_chw_to_hwc_against_float64():
    """H*W = 1, 63, 64, 65, 35*41 (one workgroup takes 64 pixels), bias given and NULL; an all-zero pixel (the 1e-12
    clamp: 0 * 1e6 = 0), a pixel of norm ~1e-7 (below the clamp, scaled by 1e6) and ordinary ones.
    DERIVED bound, ordinary pixels: the sum of 64 squares is 64 fused multiply-adds (relative error <= 64 u, halved by
    the square root), then one square root, one division and one product: the scale is off by at most
    (64 / 2 + 3) u = 35 u relatively, and outputs are at most 1 in magnitude, so |err| <= 35 * 2^-24 = 2.1e-6; with a
    bias, its float32 add contributes another u * |x + b| / norm.  Pixels under the clamp: the scale is the constant
    1 / sqrt(float32(1e-12)) (3 roundings) and |out| < 1, so the same bound holds with room."""
    import stereo_device as sd
    rng = np.random.default_rng(16)
    C = 64
    worst, worst_ratio = 0.0, 0.0
    for H, W in ((1, 1), (1, 63), (1, 64), (5, 13), (35, 41)):
        for with_bias in (False, True):
            n = H * W
            b = rng.standard_normal(C).astype(np.float32) if with_bias else None
            x = (rng.standard_normal((C, n)) * rng.choice([0.01, 1.0, 300.0], size=(1, n))).astype(np.float32)
            zero_px, tiny_px = 0, (n - 1 if n > 1 else None)
            x[:, zero_px] = -b if with_bias else 0                                  # x + b == 0 exactly
            if tiny_px is not None:
                v = rng.standard_normal(C)
                v *= 1e-7 / np.linalg.norm(v)
                x[:, tiny_px] = (v - b).astype(np.float32) if with_bias else v.astype(np.float32)
            t = x.astype(np.float64) + (b.astype(np.float64)[:, None] if with_bias else 0.0)
            S = (t * t).sum(0)
            norm = np.sqrt(np.maximum(S, np.float64(np.float32(1e-12))))
            want = (t / norm).T.reshape(H, W, C)
            assert S[zero_px] == 0 and (tiny_px is None or 0 < S[tiny_px] < 1e-13)
            ordinary = np.ones(n, bool)
            ordinary[[zero_px] + ([tiny_px] if tiny_px is not None else [])] = False
            assert (S[ordinary] > 1e-6).all()
            got = sd.l2norm_chw_to_hwc(dev(x.reshape(C, H, W)), dev(b) if with_bias else None).cpu().numpy()
            assert got.shape == (H, W, C)
            err = np.abs(got.astype(np.float64) - want)
            bound = 35 * U + (U * np.abs(want) if with_bias else 0.0)
            assert (got.reshape(n, C)[zero_px] == 0).all()
            ratio = float((err / bound).max())
            print("l2norm %dx%d bias=%d: max |err| %.3g (bound %.3g)" % (H, W, with_bias, err.max(), 35 * U))
            worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, ratio)
            assert (err <= bound).all(), "%dx%d bias=%d: |err| up to %g, %g of the derived bound" % (
                H, W, with_bias, err.max(), ratio)
            if ordinary.any():
                assert np.abs(np.linalg.norm(got.reshape(n, C)[ordinary].astype(np.float64), axis=1) - 1).max() < 1e-5
    record_measured({"l2norm_chw_to_hwc": {"bound_abs": 35 * U, "bound": "35 * 2^-24 (+ 2^-24 |x + b| / norm with a bias)",
                                           "largest_abs_error": worst, "largest_error_as_a_fraction_of_the_bound": worst_ratio}})


def test_l2norm_nan_channel_poisons_its_pixel_only():
    """np.maximum / tf.maximum keep a NaN sum of squares: the whole pixel is NaN (fmaxf would have scaled the other 63
    channels by 1e6), its neighbours are untouched."""
    import stereo_device as sd
    rng = np.random.default_rng(17)
    x = rng.standard_normal((64, 3, 43)).astype(np.float32)
    x[17, 1, 20] = np.nan
    got = sd.l2norm_chw_to_hwc(dev(x)).cpu().numpy()
    want = np.zeros((3, 43), bool)
    want[1, 20] = True
    assert np.array_equal(np.isnan(got).all(-1), want) and np.array_equal(np.isnan(got).any(-1), want)


def test_l2norm_refuses_other_channel_counts():
    import _hipabi as hip
    lib = hip.load()
    x = torch.ones((65, 4, 4), device="cuda")
    out = torch.full((4, 4, 65), 9.0, device="cuda")
    for C in (1, 63, 65):
        rc = lib.mccnn_l2norm_chw_to_hwc(hip.ptr(x), None, hip.ptr(out), C, 4, 4, hip.stream())
        assert rc == E_UNSUPPORTED and b"built for 64 feature maps" in lib.mccnn_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
