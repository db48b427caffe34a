"""CPU: the premises of the weight families of tests/accurate_reference.py (without them a pass on the GPU means
nothing), the decision kernel's operand format restated in NumPy (split_emulation) on the packing rule the kernel
shipped with and on what ACCURATE_NET.decision_layers produces now, and the pure rules behind decision_pack (the
power-of-two scale, the layer equalisation, the refusal of non-finite weights).  No device is needed."""
import functools
import math

import numpy as np
import pytest
import torch

import accurate_reference as ar
import helpers
import tolerances as tol

SEED = 11
# (H, W, D, feature maps, fc layers): both network shapes the kernel serves, a few hundred voxels each
SHAPES = {3: (3, 24, 10, 112, 3), 4: (3, 22, 8, 64, 4)}
SCORED = [(n_fc, name) for n_fc in SHAPES for name in ar.score_families(n_fc)]


@functools.lru_cache(maxsize=None)
def _inputs(n_fc):
    H, W, D, C, _ = SHAPES[n_fc]
    conv, _fc = ar.glorot_lists(C, n_fc, SEED)
    L, R = helpers.smooth_pair(H, W, seed=H + W)
    return ar.image_features_float64(conv, L).float(), ar.image_features_float64(conv, R).float(), D


@functools.lru_cache(maxsize=None)
def _family(n_fc, name):
    H, W, D, C, _ = SHAPES[n_fc]
    fl, fr, D = _inputs(n_fc)
    _conv, fc = ar.weight_family(name, C, n_fc, SEED, inputs=(fl, fr, D))
    s64, e32, e16 = ar.yardsticks(fc, fl, fr, D)
    return dict(fc=fc, s64=s64, e32=e32, e16=e16, mask=ar.valid_mask(D, H, W))


def _net_with(fc, n_fc):
    from model import ACCURATE_NET
    _H, _W, _D, C, _ = SHAPES[n_fc]
    patch = 11 if C == 112 else 9
    net = ACCURATE_NET(None, input_patch_size=patch, num_conv_layers=(patch - 1) // 2, num_conv_feature_maps=C,
                       num_fc_layers=n_fc, batch_size=1, device="cpu", seed=0)
    net.fc_weights = [w.clone() for w, _b in fc]
    net.fc_biases = [b.clone() for _w, b in fc]
    return net


def _equalised(fc, n_fc):
    """(the layers ACCURATE_NET.decision_layers hands the pack kernel, as an fc list; the scale they are packed with)."""
    import stereo_device as sd
    w, b, w_final, b_final, exps = _net_with(fc, n_fc).decision_layers()
    layers = [fc[0]] + [(w[k], b[k]) for k in range(w.shape[0])] + [(w_final[None], b_final)]
    return layers, sd.decision_weight_scale(float(w.abs().max())), exps


def _err(c, scores):
    return float(np.abs(scores - c["s64"])[c["mask"]].max())


@pytest.mark.parametrize("n_fc,name", SCORED)
def test_family_premises(n_fc, name):
    """The network is alive, the yardsticks are ordered, every float64 pre-activation is below HALF the operand limit
    (so the saturation flag must be 0 and no fallback can hide a failure), and every w >= d voxel takes part."""
    H, W, D, _C, _ = SHAPES[n_fc]
    c = _family(n_fc, name)
    fl, fr, D = _inputs(n_fc)
    assert c["e32"] > 0.0 and c["e16"] > c["e32"]
    first, hidden = ar.hidden_preactivation_max(c["fc"], fl, fr, D)
    assert first < ar.PREMISE_LIMIT and hidden < ar.PREMISE_LIMIT, (first, hidden)
    assert int(c["mask"].sum()) == H * sum(W - d for d in range(D)) and np.isfinite(c["s64"][c["mask"]]).all()
    spread = float(c["s64"][c["mask"]].max() - c["s64"][c["mask"]].min())
    if name in ar.TINY_FAMILIES:
        # hidden weights of 1e-30 and less add < 1e-27 to pre-activations of order 0.1: what is left is the biases' and
        # the final layer's score, the same in every voxel.  These families test the scale rule, not the products; the
        # bound against float64 still holds them to the right number.
        assert spread < c["e32"]
    else:
        assert spread >= 1000 * c["e32"], "%s: the scores spread by %.1f x E32 only" % (name, spread / c["e32"])


@pytest.mark.parametrize("n_fc", list(SHAPES))
def test_layer_gaps_are_the_ones_named(n_fc):
    """The gap measured from the weights is the gap the family names; the float64 scores are glorot's to the bit of
    a power-of-two rescaling (the same network function)."""
    g0 = ar.layer_maxima(_family(n_fc, "glorot")["fc"])
    assert max(g0) / min(g0) < 2.0
    names = ar.GAP_FAMILIES + ((ar.LATE_GAP_FAMILY,) if n_fc == 4 else ())
    for name in names:
        g = 2 ** int(name.split("^")[1])
        k = 1 if name == ar.LATE_GAP_FAMILY else 0
        m = ar.layer_maxima(_family(n_fc, name)["fc"])
        assert m[k] == g0[k] / g and m[k + 1] == g0[k + 1] * g, (name, m, g0)
        assert m[k + 1] / m[k] == (g0[k + 1] / g0[k]) * g * g
        c, c0 = _family(n_fc, name), _family(n_fc, "glorot")
        assert np.abs(c["s64"] - c0["s64"])[c["mask"]].max() <= 1e-15
    for name, m in (("tiny_1e-30", 1e-30), ("tiny_1e-34", 1e-34), ("tiny_1e-38", 1e-38)):
        for got in ar.layer_maxima(_family(n_fc, name)["fc"]):
            assert abs(got / m - 1.0) < 1e-6
    fc = _family(n_fc, "sparse_95")["fc"]
    for w, _b in fc[1:-1]:
        zeros = w == 0
        assert 0.94 < float(zeros.float().mean()) < 0.96
        assert bool(torch.signbit(w[zeros]).any()) and not bool(torch.signbit(w[zeros]).all())
    for name in ar.NONFINITE_FAMILIES:
        _conv, fc = ar.weight_family(name, SHAPES[n_fc][3], n_fc, SEED)
        bad = sum(int((~torch.isfinite(w)).sum()) for w, _b in fc[1:-1])
        assert bad == 1 and all(bool(torch.isfinite(w).all()) for w, _b in (fc[0], fc[-1]))
    _conv, fc = ar.weight_family("huge_1e30", SHAPES[n_fc][3], n_fc, SEED)
    assert all(abs(got / 1e30 - 1.0) < 1e-6 for got in ar.layer_maxima(fc))


@pytest.mark.parametrize("n_fc", list(SHAPES))
def test_emulation_meets_the_bound_on_glorot(n_fc):
    fl, fr, D = _inputs(n_fc)
    c = _family(n_fc, "glorot")
    s, flag = ar.split_emulation(c["fc"], fl, fr, D)
    assert flag == 0 and _err(c, s) <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    s, flag = ar.split_emulation(c["fc"], fl, fr, D, f16=True)
    assert flag == 0 and _err(c, s) <= tol.ACCURATE_F16_E16_FACTOR * c["e16"] + tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]


@pytest.mark.parametrize("n_fc,name", [(3, "gap_2^12"), (4, "gap_2^12"), (4, ar.LATE_GAP_FAMILY)])
def test_single_scale_packing_fails_the_emulation_on_a_large_gap(n_fc, name):
    """One power of two from the largest weight of ALL hidden layers, the layers as the network has them - the rule the
    kernel shipped with - loses a layer 2^24 below its neighbour: the operand format itself is far outside the bound,
    with the saturation flag down.  (If this ever passes unaided, the family no longer tests anything.)"""
    fl, fr, D = _inputs(n_fc)
    c = _family(n_fc, name)
    s, flag = ar.split_emulation(c["fc"], fl, fr, D, scale=ar.packing_rule_single_max(c["fc"]))
    err = _err(c, s)
    print("%s n_fc=%d: single-scale emulation %.1f x E32" % (name, n_fc, err / c["e32"]))
    assert flag == 0
    assert err > 10 * tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]


@pytest.mark.parametrize("n_fc,name", SCORED)
def test_equalised_operands_meet_the_bound_in_the_emulation(n_fc, name):
    """What ACCURATE_NET.decision_layers produces, packed with decision_weight_scale: the operand format meets the
    project's bounds on every family, flag 0, in both precisions."""
    fl, fr, D = _inputs(n_fc)
    c = _family(n_fc, name)
    layers, scale, exps = _equalised(c["fc"], n_fc)
    s, flag = ar.split_emulation(layers, fl, fr, D, scale=scale)
    err = _err(c, s)
    s16, flag16 = ar.split_emulation(layers, fl, fr, D, scale=scale, f16=True)
    bound16 = tol.ACCURATE_F16_E16_FACTOR * c["e16"] + tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    print("%s n_fc=%d: log2 c = %s, emulation %.2f x E32, f16 %.2f of its bound" % (
        name, n_fc, exps, err / c["e32"], _err(c, s16) / bound16))
    assert flag == 0 and flag16 == 0
    assert err <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    assert _err(c, s16) <= bound16


@pytest.mark.parametrize("n_fc,name", SCORED)
def test_equalisation_is_exact(n_fc, name):
    """The equalised layers are the network's times exact powers of two (glorot: the same bits, c = 1), every hidden
    layer's largest weight in one binade, and the float64 scores of the equalised layers are the network's."""
    fl, fr, D = _inputs(n_fc)
    c = _family(n_fc, name)
    layers, scale, exps = _equalised(c["fc"], n_fc)
    prev = 0
    for k, ((w, b), (w0, b0)) in enumerate(zip(layers[1:-1], c["fc"][1:-1])):
        assert torch.equal(w.double(), w0.double() * 2.0 ** (exps[k] - prev))
        assert torch.equal(b.double(), b0.double() * 2.0 ** exps[k])
        prev = exps[k]
    assert torch.equal(layers[-1][0].double().reshape(-1), c["fc"][-1][0].double().reshape(-1) * 2.0 ** -prev)
    m = ar.layer_maxima(layers)
    assert len({math.frexp(x)[1] for x in m}) == 1, m
    assert 512.0 < max(m) * scale <= 1024.0 or name in ("tiny_1e-34", "tiny_1e-38")
    if name == "glorot":
        assert exps == [0] * (n_fc - 1)
    if name not in ar.TINY_FAMILIES:        # (float64 on the equalised float32 layers: exact up to float64 rounding)
        s = ar.scores(layers, fl, fr, D)
        assert np.abs(s - c["s64"])[c["mask"]].max() <= 1e-13


def test_scale_rule_is_finite_for_every_float32_maximum():
    """A finite, positive, normal float32 whose x 256 and whose reciprocal of that are finite and normal too, for
    max |w| from float32's smallest subnormal to its largest number; m * scale in (512, 1024] wherever no clamp acts."""
    import stereo_device as sd
    tiny = float(np.finfo(np.float32).tiny)
    ms = [1e-45, 1.4e-45, 1e-40, 1e-38, 7.7e-34, 3e-36, 1e-34, 1e-30, 1e-10, 0.0884, 1.0, 1023.9, 1024.0, 2048.0, 1e30,
          3.4e38, float(np.finfo(np.float32).max)] + [float(x) for x in 10.0 ** np.linspace(-45, 38.5, 400)]
    for m in ms:
        m = float(np.float32(m))
        if m == 0.0:
            continue
        s = sd.decision_weight_scale(m)
        with np.errstate(over="raise", under="raise"):
            s32 = np.float32(s)
            s256 = np.float32(s32 * np.float32(256.0))
            inv = np.float32(1.0) / s256
        assert float(s32) == s and math.frexp(s)[0] == 0.5, m           # a power of two, exactly a float32
        for v in (s32, s256, inv):
            assert np.isfinite(v) and float(v) >= tiny, (m, v)
        if 11 - math.frexp(m)[1] < sd.DECISION_SCALE_MAX_EXP:
            assert 512.0 < m * s <= 1024.0, m
        else:
            assert m * s <= 1024.0
    assert sd.decision_weight_scale(0.0) == 1.0
    # the rule the kernel shipped with, where it was sound
    for m in (0.0884, 1.0, 0.5, 1024.0, 3.3, 1e-20, 1e20):
        assert sd.decision_weight_scale(m) == 2.0 ** math.floor(math.log2(1024.0 / m))


def test_non_finite_weights_are_refused():
    """decision_weight_scale and decision_equalise_exponents refuse inf and NaN maxima (the earlier rule packed them with
    scale 1, clamped to +-65504: a finite wrong score, no flag); decision_layers names the layer."""
    import _hipabi as hip
    import stereo_device as sd
    for bad in (float("inf"), float("-inf"), float("nan"), -1.0):
        with pytest.raises(ValueError, match="finite"):
            sd.decision_weight_scale(bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="fc3"):
            sd.decision_equalise_exponents([0.1, bad])
    for name in ar.NONFINITE_FAMILIES:
        for n_fc in SHAPES:
            _conv, fc = ar.weight_family(name, SHAPES[n_fc][3], n_fc, SEED)
            layer = [k + 1 for k, (w, _b) in enumerate(fc) if not bool(torch.isfinite(w).all())]
            with pytest.raises(hip.MccnnHipError, match="fc%d" % layer[0]):
                _net_with(fc, n_fc).decision_layers()


def test_equalise_exponents_rule():
    import stereo_device as sd
    eq = sd.decision_equalise_exponents
    assert eq([0.08, 0.07]) == [0, 0] and eq([0.08, 0.07, 0.09]) == [0, 0, 0]
    assert eq([0.08 / 4096, 0.08 * 4096]) == [12, 0]
    assert eq([0.08, 0.08 / 4096, 0.08 * 4096]) == [0, 12, 0]
    assert eq([0.0, 0.0]) == [0, 0] and eq([0.0, 0.3]) == [0, 0] and eq([1e-38, 1e-38]) == [0, 0]
    # the clamp: partial, still a list of integers within +-DECISION_EQUALISE_MAX_EXP
    out = eq([1e-38, 1e38])
    assert all(abs(c) <= sd.DECISION_EQUALISE_MAX_EXP for c in out) and out[0] == sd.DECISION_EQUALISE_MAX_EXP
    # the product of the layer gains is kept to within half a binade per layer
    for ms in ([3.0, 0.001, 17.0], [1e-5, 2e-5], [0.5, 0.25, 1e3]):
        assert abs(eq(ms)[-1]) <= len(ms)
