"""GPU: the accurate network's decision stage (csrc/decision_mfma.hip and the library route) and the whole pair behind
it, against the float64 restatements of tests/accurate_reference.py.  Bounds (src/tolerances.py) are multiples of two
errors computed here, on the same inputs: E32 (a float32 torch-CPU evaluation) and E16 (a float64 evaluation with
weights and every layer's input rounded to f16).  Every voxel takes part in every comparison; each device step runs
once (results are shared between the tests through _volumes / _case)."""
import functools
import re
import warnings

import numpy as np
import pytest
import torch

import accurate_reference as ar
import helpers
import tolerances as tol

pytestmark = pytest.mark.gpu

# name -> (H, W, D, feature maps, fc layers, patch, scale of the last layer)
CASES = {
    "4x9x2": (4, 9, 2, 112, 3, 11, 1.0),
    "5x67x33": (5, 67, 33, 112, 3, 11, 1.0),
    "24x100x64": (24, 100, 64, 112, 3, 11, 1.0),
    "3x130x128": (3, 130, 128, 112, 3, 11, 1.0),
    "8x300x256": (8, 300, 256, 112, 3, 11, 1.0),
    "kitti_6x70x40": (6, 70, 40, 64, 4, 9, 1.0),
    "saturated_5x67x33": (5, 67, 33, 112, 3, 11, 8.0),
    # (with glorot weights the logits are small: x 8 moves the scores to 0.46 .. 0.48 only; x 512 reaches an end)
    "ends_5x67x33": (5, 67, 33, 112, 3, 11, 512.0),
}
LAYOUTS = ("pixel_major", "plane_major")


def _check_tower(net, images, feats, what):
    """The whole-image tower on the GPU (library convolutions at C maps, bias + ReLU after EVERY layer, NCHW -> NHWC)
    against the float64 restatement from the images: zero-padded once, no normalisation."""
    conv, _fc = ar.net_lists(net)
    worst = 0.0
    for img, f in zip(images, feats):
        want = ar.image_features_float64(conv, img.detach().cpu()).numpy()
        assert tuple(f.shape) == want.shape, "%s: features are %s, expected %s" % (what, tuple(f.shape), want.shape)
        worst = max(worst, float(np.abs(f.detach().cpu().numpy().astype(np.float64) - want).max()))
    print("%s: tower max err %.3e against float64 (largest feature %.2f)" % (what, worst, float(np.abs(want).max())))
    assert worst <= tol.FEATURES_ABS, "%s: whole-image tower differs from float64 by %g" % (what, worst)


def _make_net(C, n_fc, patch, last_scale, seed=11):
    from model import ACCURATE_NET
    net = ACCURATE_NET(None, input_patch_size=patch, num_conv_layers=(patch - 1) // 2, num_conv_feature_maps=C,
                       num_fc_layers=n_fc, batch_size=1, device="cuda", seed=seed)      # seeded glorot
    if last_scale != 1.0:
        net.fc_weights[-1] = net.fc_weights[-1] * last_scale
        net.fc_biases[-1] = net.fc_biases[-1] * last_scale
    return net


@functools.lru_cache(maxsize=None)
def _case(name):
    """The network, its tower outputs on a smooth pair (the decision stage's inputs) and the yardsticks on them."""
    H, W, D, C, n_fc, patch, last_scale = CASES[name]
    net = _make_net(C, n_fc, patch, last_scale)
    L, R = (t.cuda() for t in helpers.smooth_pair(H, W, seed=H + W))
    fl, fr = net.features_pair_hwc(L, R)
    torch.cuda.synchronize()
    _check_tower(net, (L, R), (fl, fr), name)
    _conv, fc = ar.net_lists(net)
    s64, e32, e16 = ar.yardsticks(fc, fl.cpu(), fr.cpu(), D)
    assert e32 > 0.0 and e16 > e32
    return dict(net=net, fl=fl, fr=fr, D=D, s64=s64, e32=e32, e16=e16, mask=ar.valid_mask(D, H, W), images=(L, R))


@functools.lru_cache(maxsize=None)
def _volumes(name, layout, decision, mode):
    """(lcv, rcv) float32 [D,H,W] on the host + the saturation flag, from ONE call of cost_volume_accurate."""
    import stereo_device as sd
    c = _case(name)
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    pm = layout == "pixel_major"
    lcv, rcv = sd.cost_volume_accurate(c["net"], c["fl"], c["fr"], c["D"], mode=mode, decision=decision, pixel_major=pm,
                                       sat_flag=flag if decision == "kernel" else None)
    torch.cuda.synchronize()
    if pm:
        lcv, rcv = sd.hwd_to_dhw(lcv, c["D"]), sd.hwd_to_dhw(rcv, c["D"])
    return lcv.cpu().numpy(), rcv.cpu().numpy(), int(flag.item())


def _score_error(name, lcv):
    c = _case(name)
    return float(np.abs(-lcv.astype(np.float64) - c["s64"])[c["mask"]].max())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_scores_default_precision(name, layout):
    """Split operands: every w >= d score within 4 x E32 of the float64 restatement."""
    import _hipabi as hip
    c = _case(name)
    lcv, _rcv, flag = _volumes(name, layout, "kernel", hip.MCCNN_CV_EXACT)
    err = _score_error(name, lcv)
    print("%s %s: split kernel max err %.3e, E32 %.3e, ratio %.2f" % (name, layout, err, c["e32"], err / c["e32"]))
    assert flag == 0
    assert np.isfinite(lcv).all()
    assert err <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    if name.startswith("ends"):
        s = -lcv[c["mask"]]
        assert (s < 1e-3).any() or (s > 1 - 1e-3).any(), "the case was meant to drive the sigmoid to its ends"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_scores_f16_precision(name, layout):
    """One f16 product per multiply: within 2 x E16 + 4 x E32."""
    import _hipabi as hip
    c = _case(name)
    lcv, _rcv, flag = _volumes(name, layout, "kernel", hip.MCCNN_CV_MFMA)
    err = _score_error(name, lcv)
    bound = tol.ACCURATE_F16_E16_FACTOR * c["e16"] + tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    print("%s %s: f16 kernel max err %.3e, E16 %.3e, bound %.3e" % (name, layout, err, c["e16"], bound))
    assert flag == 0
    assert err <= bound


@pytest.mark.parametrize("decision", ("kernel", "library"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_borders_and_right_volume_bit_identical(name, layout, decision):
    """The border recurrences and the right-volume copy, restated literally in float32 and applied to the GPU's own
    w >= d scores, give both volumes bit for bit."""
    import _hipabi as hip
    lcv, rcv, _flag = _volumes(name, layout, decision, hip.MCCNN_CV_EXACT)
    want_l, want_r = ar.volumes_from_scores(lcv)
    helpers.assert_bits_strict(lcv, want_l, "%s %s %s: left volume" % (name, layout, decision))
    helpers.assert_bits_strict(rcv, want_r, "%s %s %s: right volume" % (name, layout, decision))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_and_library_routes_agree(name, layout):
    import _hipabi as hip
    c = _case(name)
    k = _volumes(name, layout, "kernel", hip.MCCNN_CV_EXACT)[0]
    l = _volumes(name, layout, "library", hip.MCCNN_CV_EXACT)[0]
    lib_err = _score_error(name, l)
    print("%s %s: library max err %.3e (%.2f x E32)" % (name, layout, lib_err, lib_err / c["e32"]))
    assert lib_err <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    assert float(np.abs(k.astype(np.float64) - l)[c["mask"]].max()) <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]


@pytest.mark.parametrize("precision", ("split", "f16"))
def test_operand_saturation_raises_the_flag(precision):
    """An activation beyond the f16 range of the operands (|x| >= 255.9) of a stored voxel sets the flag - the contract
    of the split-operand feature kernels - in either precision; the volumes stay finite (the operand is clamped)."""
    import _hipabi as hip
    import stereo_device as sd
    c = _case("5x67x33")
    mode = hip.MCCNN_CV_EXACT if precision == "split" else hip.MCCNN_CV_MFMA
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    lcv, rcv = sd.cost_volume_accurate(c["net"], c["fl"] * 4000.0, c["fr"] * 4000.0, c["D"], mode=mode,
                                       decision="kernel", sat_flag=flag)
    assert int(flag.item()) == 1
    assert bool(torch.isfinite(lcv[:, :, :c["D"]]).all()) and bool(torch.isfinite(rcv[:, :, :c["D"]]).all())
    # and the same inputs at their own scale leave it alone
    flag.zero_()
    sd.cost_volume_accurate(c["net"], c["fl"], c["fr"], c["D"], mode=mode, decision="kernel", sat_flag=flag)
    assert int(flag.item()) == 0


def test_matcher_on_saturation():
    """A pair whose first fully-connected layer exceeds the operands' range: 'fallback' (default) returns the map of the
    library decision route, 'raise' raises and names the decision kernel, 'ignore' leaves the flag to the caller."""
    import stereo_device as sd
    import synthetic
    H, W, D = 12, 48, 16
    net = _make_net(112, 3, 11, 1.0)
    net.fc_weights[0] = net.fc_weights[0] * 4000.0
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=9)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    want = sd.StereoMatcher(net, decision="library").match(dl, dr, D).cpu().numpy()
    m = sd.StereoMatcher(net, decision="kernel")
    assert m.on_saturation == "fallback" and m._library_twin is None
    got = m.match(dl, dr, D).cpu().numpy()
    assert m._library_twin is not None and m._library_twin.decision == "library"
    helpers.assert_bits_strict(got, want, "on_saturation='fallback'")
    assert not m.features_saturated()                        # read and reset by the fallback
    helpers.assert_bits_strict(m.match_graph(dl, dr, D).cpu().numpy(), want, "on_saturation='fallback' (graph replay)")
    with pytest.raises(RuntimeError, match="decision kernel"):
        sd.StereoMatcher(net, decision="kernel", on_saturation="raise").match(dl, dr, D)
    loose = sd.StereoMatcher(net, decision="kernel", on_saturation="ignore")
    loose.match(dl, dr, D)
    assert loose._library_twin is None and loose.features_saturated() and not loose.features_saturated()
    assert "decision kernel" in loose.saturation_notice() and "{}" in loose.saturation_notice()


@pytest.mark.parametrize("name", ["24x100x64", "8x300x256"])
def test_whole_pair(name):
    """StereoMatcher on an ACCURATE_NET: the kept cost volume meets the score bound, every later stage is the CPU
    checker's bit for bit on the GPU's own previous output, and the graph replay equals the eager map."""
    import oracle as o
    import stereo_device as sd
    import synthetic
    H, W, D, C, n_fc, patch, last_scale = CASES[name]
    net = _make_net(C, n_fc, patch, last_scale)
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=5)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = sd.StereoMatcher(net, decision="kernel")
    assert m.accurate and m.features == "miopen"
    keep = {}
    out = m.match(dl, dr, D, keep=keep)
    torch.cuda.synchronize()
    assert m.saturation_checked() and not m.features_saturated()
    # check 1 on the kept volume, from the same tower outputs
    fl, fr = net.features_pair_hwc(dl[:, :, 0].contiguous(), dr[:, :, 0].contiguous())
    _check_tower(net, (dl[:, :, 0], dr[:, :, 0]), (fl, fr), "%s whole pair" % name)
    _conv, fc = ar.net_lists(net)
    s64, e32, _e16 = ar.yardsticks(fc, fl.cpu(), fr.cpu(), D)
    mask = ar.valid_mask(D, H, W)
    cv_l, cv_r = (t.cpu().numpy() for t in keep["cv"])
    err = float(np.abs(-cv_l.astype(np.float64) - s64)[mask].max())
    print("%s whole pair: cost volume max err %.3e, E32 %.3e" % (name, err, e32))
    assert err <= tol.ACCURATE_SPLIT_E32_FACTOR * e32
    want_l, want_r = ar.volumes_from_scores(cv_l)
    helpers.assert_bits_strict(cv_l, want_l, "kept left volume")
    helpers.assert_bits_strict(cv_r, want_r, "kept right volume")
    d = helpers.stagewise(keep, L, R, D, o, hp=m.hp)
    assert helpers.first_differing_stage(d) is None, d
    helpers.assert_bits_strict(out.cpu().numpy(), keep["bilateral"].cpu().numpy(), "returned map")
    eager = m.match(dl, dr, D).cpu().numpy()
    helpers.assert_bits_strict(eager, out.cpu().numpy(), "match() without keep")
    graph = m.match_graph(dl, dr, D).cpu().numpy()
    helpers.assert_bits_strict(graph, eager, "match_graph against match")
    # the library route through the matcher: same volumes within the bound, nothing else moves
    ml = sd.StereoMatcher(net, decision="library")
    keep_l = {}
    ml.match(dl, dr, D, keep=keep_l)
    lib = keep_l["cv"][0].cpu().numpy()
    assert float(np.abs(lib.astype(np.float64) - cv_l)[mask].max()) <= tol.ACCURATE_SPLIT_E32_FACTOR * e32
    assert helpers.first_differing_stage(helpers.stagewise(keep_l, L, R, D, o, hp=ml.hp)) is None


def test_fast_network_unchanged_in_the_same_process(net_layers):
    """A fast-network matcher created after an accurate one still gives the CPU checker's stages and final map."""
    import oracle as o
    import stereo_device as sd
    import synthetic
    from model import NET
    acc = sd.StereoMatcher(_make_net(112, 3, 11, 1.0))
    L0, R0, _, _, _ = synthetic.make_pair(12, 40, 8, seed=2)
    acc.match(torch.from_numpy(L0).cuda(), torch.from_numpy(R0).cuda(), 8)
    H, W, D = 48, 64, 16
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=3)
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    m = sd.StereoMatcher(net)
    assert not m.accurate
    keep = {}
    out = m.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), D, keep=keep)
    fl, fr = net.features_pair_hwc_split(torch.from_numpy(L[:, :, 0]).cuda(), torch.from_numpy(R[:, :, 0]).cuda())
    d = helpers.stagewise(keep, L, R, D, o, hp=m.hp, features=(fl, fr))
    assert helpers.first_differing_stage(d) is None, d
    db = o.bilateral_filter(L, keep["median"].cpu().numpy(), 5, 5, 0, 6, 2)
    helpers.assert_bits_strict(out.cpu().numpy(), db, "fast network: final map")


def test_refusals_name_the_limit():
    """C = 96, 256 units and D = W - 1 are refused before anything is launched; decision='auto' falls back to the
    library route with a warning that names the reason."""
    import _hipabi as hip
    import stereo_device as sd
    from model import ACCURATE_NET
    H, W = 6, 40
    for kw, D, needle in ((dict(num_conv_feature_maps=96), 16, "96 feature maps"),
                          (dict(num_fc_units=256), 16, "256 units"),
                          (dict(), W - 1, "ndisp + 2")):
        net = ACCURATE_NET(None, batch_size=1, device="cuda", seed=1, **kw)
        C = net.num_conv_feature_maps
        fl = torch.rand((H, W, C), device="cuda")
        fr = torch.rand((H, W, C), device="cuda")
        out = tuple(torch.full((H, W, sd.hwd_pitch(D)), 5.0, device="cuda") for _ in range(2))
        with pytest.raises(hip.MccnnHipError, match=re.escape(needle)):
            sd.cost_volume_accurate(net, fl, fr, D, decision="kernel", out=out)
        torch.cuda.synchronize()
        assert bool((out[0] == 5.0).all()) and bool((out[1] == 5.0).all())       # nothing was launched
        with pytest.raises(ValueError, match=re.escape(needle)):
            sd.StereoMatcher(net, decision="kernel").decision_route(W, D)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            assert sd.StereoMatcher(net, decision="auto").decision_route(W, D) == "library"
        assert any(needle in str(w.message) for w in rec)
    # the entry point itself, with real buffers: refused, volumes untouched
    lib = hip.load()
    net = ACCURATE_NET(None, batch_size=1, device="cuda", seed=1)
    D = 16
    a = torch.rand((H, W, 384), device="cuda")
    packed, scale, biases, w_final, b_final = net.decision_operands(hip.MCCNN_CV_EXACT)
    vol = torch.full((H, W, sd.hwd_pitch(D)), 5.0, device="cuda")
    rc = lib.mccnn_cost_volume_accurate_hwd(hip.ptr(a), hip.ptr(a), H, W, 96, 384, 3, D, hip.ptr(packed), hip.ptr(biases),
                                            hip.ptr(w_final), b_final, scale, hip.ptr(vol), hip.ptr(vol), 0, None,
                                            hip.stream())
    assert rc == hip.MCCNN_E_UNSUPPORTED and b"64 or 112" in lib.mccnn_last_error_string()
    torch.cuda.synchronize()
    assert bool((vol == 5.0).all())


def test_process_functional_accurate():
    """compute_features accepts the accurate model and compute_cost_volume_accurate sits beside compute_cost_volume."""
    import process_functional as pf
    c = _case("5x67x33")
    L, R = c["images"]
    fl, fr = pf.compute_features(L.cpu().numpy()[:, :, None], R.cpu().numpy()[:, :, None], 11, 11, c["net"])
    assert isinstance(fl, np.ndarray) and fl.shape == (5, 67, 112) and fl.min() >= 0.0
    # (one view per call here, both as one batch in _case: the library may pick another convolution kernel)
    assert np.abs(fl - c["fl"].cpu().numpy()).max() <= tol.FEATURES_ABS
    assert np.abs(fr - c["fr"].cpu().numpy()).max() <= tol.FEATURES_ABS
    lcv, rcv = pf.compute_cost_volume_accurate(c["fl"].cpu().numpy(), c["fr"].cpu().numpy(), c["D"],
                                               c["net"].get_fc_layers())
    assert isinstance(lcv, np.ndarray) and lcv.shape == (c["D"], 5, 67) and rcv.shape == lcv.shape
    assert _score_error("5x67x33", lcv) <= tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    want_l, want_r = ar.volumes_from_scores(lcv)
    helpers.assert_bits_strict(rcv, want_r, "compute_cost_volume_accurate: right volume")
    # checkpoint arrays edited in place are seen (the packed weights are keyed on content, not on the arrays' identity)
    fc = c["net"].get_fc_layers()
    args = (c["fl"].cpu().numpy(), c["fr"].cpu().numpy(), c["D"])
    first, _ = pf.compute_cost_volume_accurate(*args, fc)
    helpers.assert_bits_strict(first, lcv, "compute_cost_volume_accurate: same weights, new arrays")
    fc[-1][1][...] += 1.5
    fc[1][0][...] *= 0.5
    edited, _ = pf.compute_cost_volume_accurate(*args, fc)
    other = _make_net(*CASES["5x67x33"][3:])
    other.set_layers(other.get_layers(), fc)
    want, _ = pf.compute_cost_volume_accurate(*args, other)
    helpers.assert_bits_strict(edited, want, "compute_cost_volume_accurate: arrays edited in place")
    assert not helpers.bits_strict(edited, first)
