"""GPU: the decision kernel (csrc/decision_mfma.hip) where tests/test_accurate_gpu.py does not reach.
  (a) what raises the saturation flag - NaN of either sign, +inf, the first value above 255.875 - and what does not
      (255.875 itself, -inf), in aL, in aR and in the hidden layers, isolated from the scores by a unit whose outgoing
      weights are zero: every stored score must stay the clean run's bit for bit;
  (b) the flag counts stored voxels only: lanes that store nothing (d >= D, w >= W) see 300 and must stay silent;
  (c) D = 513, 769, 1024 (disparity blocks 8 .. 31): scores on a sample that holds every seam of the tiling
      (accurate_reference.sample_voxels) against float64, EVERY valid voxel against the library route, borders, layouts;
  (d) entries the call must not write: the Dp - D pad entries of a pixel, the plane behind the last one;
  (e) a NaN image through StereoMatcher: the pair is repeated on the library route and comes back as its NaN.
Each device step runs once (results are shared between the tests through lru_cache)."""
import functools

import numpy as np
import pytest
import torch

import accurate_reference as ar
import helpers
import tolerances as tol
from test_accurate_gpu import _check_tower, _make_net

pytestmark = pytest.mark.gpu

LAYOUTS = ("pixel_major", "plane_major")
PRECISIONS = ("split", "f16")


def _mode(precision):
    import _hipabi as hip
    return hip.MCCNN_CV_EXACT if precision == "split" else hip.MCCNN_CV_MFMA


def _launch(net, aL, aR, D, precision, layout, out=None):
    """The entry point itself on the two halves [H,W,units]: (lcv, rcv, flag) - volumes in the layout's own shape
    ([H,W,Dp] / [D,H,W], zero-filled unless `out` is given), the flag as an int."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W, U = aL.shape
    mode = _mode(precision)
    pm = layout == "pixel_major"
    if out is None:
        shape = (H, W, sd.hwd_pitch(D)) if pm else (D, H, W)
        out = tuple(torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(2))
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    packed, scale, biases, w_final, b_final = net.decision_operands(mode)
    fn = lib.mccnn_cost_volume_accurate_hwd if pm else lib.mccnn_cost_volume_accurate
    hip.check(fn(hip.ptr(aL), hip.ptr(aR), H, W, net.num_conv_feature_maps, U, net.num_fc_layers, D, hip.ptr(packed),
                 hip.ptr(biases), hip.ptr(w_final), b_final, scale, hip.ptr(out[0]), hip.ptr(out[1]), mode,
                 hip.ptr(flag), hip.stream()), "mccnn_cost_volume_accurate*")
    torch.cuda.synchronize()
    return out[0], out[1], int(flag.item())


def _bits(value):
    """The int32 pattern of a value as float32 (a NaN's sign bit included when it comes as a numpy float32)."""
    return int(np.array([value], dtype=np.float32).view(np.int32)[0])


def _put(t, index, value):
    """t[index] = value, written as its bit pattern."""
    t.view(torch.int32)[index] = _bits(value)


def _stored_bits(vol, D, layout):
    """The d < D entries of a volume as int32, on the host."""
    v = vol[:, :, :D] if layout == "pixel_major" else vol[:D]
    return v.contiguous().view(torch.int32).cpu().numpy()


# ---- (a), (b): the flag, on 3 x 41 x 19 (Dp = 20, D % 32 != 0, W % 4 = 1) ------------------------------------------
FH, FW, FD = 3, 41, 19
U0, U1, U2 = 77, 203, 310      # units of the first, second and third hidden layer whose outgoing weights are zeroed
ABOVE = float(np.nextafter(np.float32(255.875), np.float32(np.inf)))
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]       # kept as a float32: the sign must survive
FLAG_VALUES = {                # name -> (value, expected flag)
    "nan": (float("nan"), 1),
    "plus_inf": (float("inf"), 1),
    "above_255.875": (ABOVE, 1),
    "exactly_255.875": (255.875, 0),
    "minus_inf": (float("-inf"), 0),
    "minus_nan": (NEG_NAN, 1),
}


@functools.lru_cache(maxsize=None)
def _flag_case():
    """A 112-map, 3-layer network whose units U0 (first hidden layer), U1 (second) and U2 (third) reach nothing
    downstream, and the halves of a smooth pair with unit U0 cleared."""
    assert FD % 32 != 0 and FW % 4 == 1
    net = _make_net(112, 3, 11, 1.0)
    with torch.no_grad():
        net.fc_weights[1][:, U0] = 0.0
        net.fc_weights[2][:, U1] = 0.0
        net.fc_weights[3][:, U2] = 0.0
    L, R = (t.cuda() for t in helpers.smooth_pair(FH, FW, seed=FH + FW))
    fl, fr = net.features_pair_hwc(L, R)
    aL, aR = net.first_layer_halves(fl, fr)
    aL[:, :, U0] = 0.0
    aR[:, :, U0] = 0.0
    torch.cuda.synchronize()
    assert float(aL.abs().max()) < 100.0 and float(aR.abs().max()) < 100.0       # far inside the range
    return dict(net=net, aL=aL, aR=aR)


@functools.lru_cache(maxsize=None)
def _flag_clean(layout, precision):
    import stereo_device as sd
    c = _flag_case()
    lcv, rcv, flag = _launch(c["net"], c["aL"], c["aR"], FD, precision, layout)
    assert flag == 0
    if layout == "pixel_major":
        assert sd.hwd_pitch(FD) == 20
    l, r = _stored_bits(lcv, FD, layout), _stored_bits(rcv, FD, layout)
    assert np.isfinite(l.view(np.float32)).all() and np.isfinite(r.view(np.float32)).all()
    return l, r


def _assert_clean(lcv, rcv, layout, precision, what):
    want_l, want_r = _flag_clean(layout, precision)
    assert np.array_equal(_stored_bits(lcv, FD, layout), want_l), "%s: the left volume moved" % what
    assert np.array_equal(_stored_bits(rcv, FD, layout), want_r), "%s: the right volume moved" % what


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(FLAG_VALUES))
def test_flag_of_one_value_in_a_half(name, layout, precision):
    """One value in unit U0 of aL at one pixel, then of aR at one pixel (the partner's unit is 0: the sum is the value).
    NaN of either sign, +inf and the first float above 255.875 raise the flag; 255.875 and -inf (relu: 0, as on the
    library route) do not; the unit reaches nothing, so both volumes are the clean run's bit for bit in every case."""
    value, want = FLAG_VALUES[name]
    c = _flag_case()
    _flag_clean(layout, precision)
    for side, (h, w) in (("aL", (1, FW - 1)), ("aR", (2, 7))):      # aL: a pixel of the ragged last workgroup
        halves = {"aL": c["aL"], "aR": c["aR"]}
        bad = halves[side].clone()
        _put(bad, (h, w, U0), value)
        if name == "minus_nan":
            assert int(bad.view(torch.int32)[h, w, U0]) == 0xffc00000 - (1 << 32)
        halves[side] = bad
        lcv, rcv, flag = _launch(c["net"], halves["aL"], halves["aR"], FD, precision, layout)
        what = "%s in %s[%d,%d] (%s, %s)" % (name, side, h, w, layout, precision)
        print("%s: flag %d, expected %d" % (what, flag, want))
        assert flag == want, what
        _assert_clean(lcv, rcv, layout, precision, what)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_flag_of_one_value_in_a_hidden_layer(layout, precision):
    """The same through a bias: a hidden layer that feeds f16 operands flags NaN and what is above the range, and lets
    -inf pass; the last hidden layer feeds the float32 final product: it has no range and flags NaN alone."""
    c = _flag_case()
    net = c["net"]
    _flag_clean(layout, precision)
    rows = ((1, U1, float("nan"), 1), (1, U1, NEG_NAN, 1), (1, U1, 300.0, 1), (1, U1, float("inf"), 1),
            (1, U1, float("-inf"), 0), (2, U2, float("nan"), 1), (2, U2, NEG_NAN, 1), (2, U2, 300.0, 0),
            (2, U2, float("-inf"), 0))
    for layer, unit, value, want in rows:
        before = net.fc_biases[layer][unit].item()
        try:
            with torch.no_grad():
                _put(net.fc_biases[layer], unit, value)
            lcv, rcv, flag = _launch(net, c["aL"], c["aR"], FD, precision, layout)
        finally:
            with torch.no_grad():
                _put(net.fc_biases[layer], unit, before)
        what = "bias %r in unit %d of fc%d (%s, %s)" % (value, unit, layer + 1, layout, precision)
        print("%s: flag %d, expected %d" % (what, flag, want))
        assert flag == want, what
        _assert_clean(lcv, rcv, layout, precision, what)
    lcv, rcv, flag = _launch(net, c["aL"], c["aR"], FD, precision, layout)       # the biases are back
    assert flag == 0
    _assert_clean(lcv, rcv, layout, precision, "restored biases")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_flag_counts_stored_voxels_only(layout, precision):
    """Unit U0 is 150 in aR[h, 0], in aL[h, w] for w >= D (W - 1 among them) and 0 elsewhere: every stored voxel sees
    at most 150, and only lanes that store nothing - D <= d inside the last 32-block and w >= W, which read aR at
    column 0 - see 300.  The flag stays 0 and the volumes are the clean run's."""
    c = _flag_case()
    aL, aR = c["aL"].clone(), c["aR"].clone()
    aR[:, 0, U0] = 150.0
    aL[:, FD:, U0] = 150.0
    assert float(aL[:, FW - 1, U0].min()) == 150.0
    for d in range(FD):                                                 # the premise: no stored voxel is beyond 150
        assert float((aL[:, d:, U0] + aR[:, :FW - d, U0]).max()) <= 150.0
    assert float((aL[:, FW - 1, U0] + aR[:, 0, U0]).min()) == 300.0     # what an unstored lane adds up
    lcv, rcv, flag = _launch(c["net"], aL, aR, FD, precision, layout)
    assert flag == 0, "a lane that stores nothing raised the flag"
    _assert_clean(lcv, rcv, layout, precision, "unstored lanes at 300 (%s, %s)" % (layout, precision))


# ---- (c): D up to 1024 -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_case(name):
    H, W, D, C, n_fc, patch = ar.EDGE_CASES[name]
    net = _make_net(C, n_fc, patch, 1.0)
    L, R = (t.cuda() for t in helpers.smooth_pair(H, W, seed=H + W))
    fl, fr = net.features_pair_hwc(L, R)
    torch.cuda.synchronize()
    _check_tower(net, (L, R), (fl, fr), name)
    _conv, fc = ar.net_lists(net)
    sample = ar.edge_sample(name)
    assert len(sample[0]) <= ar.EDGE_SAMPLE_CAP
    s64, e32, e16 = ar.sampled_yardsticks(fc, fl.cpu(), fr.cpu(), sample)
    print("%s: %d sampled voxels, E32 %.3e, E16 %.3e" % (name, len(s64), e32, e16))
    assert e32 > 0.0 and e16 > e32
    return dict(net=net, fl=fl, fr=fr, H=H, W=W, D=D, sample=sample, s64=s64, e32=e32, e16=e16,
                mask=ar.valid_mask(D, H, W))


@functools.lru_cache(maxsize=None)
def _edge_volumes(name, layout, route):
    """(lcv, rcv) float32 [D,H,W] on the host + the flag from ONE call; route: 'split', 'f16' (kernel) or 'library'."""
    import _hipabi as hip
    import stereo_device as sd
    c = _edge_case(name)
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    pm = layout == "pixel_major"
    kernel = route != "library"
    lcv, rcv = sd.cost_volume_accurate(c["net"], c["fl"], c["fr"], c["D"], mode=_mode(route) if kernel else
                                       hip.MCCNN_CV_EXACT, decision="kernel" if kernel else "library", pixel_major=pm,
                                       sat_flag=flag if kernel else None)
    torch.cuda.synchronize()
    if pm:
        assert lcv.shape[2] == sd.hwd_pitch(c["D"])
        lcv, rcv = sd.hwd_to_dhw(lcv, c["D"]), sd.hwd_to_dhw(rcv, c["D"])
    return lcv.cpu().numpy(), rcv.cpu().numpy(), int(flag.item())


def _sample_error(name, lcv):
    c = _edge_case(name)
    h, w, d = c["sample"]
    return float(np.abs(-lcv[d, h, w].astype(np.float64) - c["s64"]).max())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(ar.EDGE_CASES))
def test_large_d_scores_on_the_sample(name, layout):
    """The bounds of src/tolerances.py with the yardsticks of the same sample: split kernel and library route within
    4 x E32 of float64, f16 kernel within 2 x E16 + 4 x E32; no flag, finite volumes."""
    c = _edge_case(name)
    b32 = tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    b16 = tol.ACCURATE_F16_E16_FACTOR * c["e16"] + b32
    errs = {}
    for route in ("split", "f16", "library"):
        lcv, rcv, flag = _edge_volumes(name, layout, route)
        errs[route] = _sample_error(name, lcv)
        assert flag == 0, route
        assert np.isfinite(lcv).all() and np.isfinite(rcv).all(), route
    print("%s %s: split %.3e (%.2f x E32), library %.3e (%.2f x E32), f16 %.3e (bound %.3e)" % (
        name, layout, errs["split"], errs["split"] / c["e32"], errs["library"], errs["library"] / c["e32"], errs["f16"],
        b16))
    assert errs["split"] <= b32
    assert errs["library"] <= b32
    assert errs["f16"] <= b16


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(ar.EDGE_CASES))
def test_large_d_every_voxel_against_the_library_route(name, layout):
    """EVERY w >= d voxel: both routes meet 4 x E32 against float64, so they are within 2 x 4 x E32 of each other; a
    voxel written to a neighbour's place is ten times beyond that (tests/test_accurate_edges_cpu.py).  The f16 kernel
    under the sum of its bound and the library's, by the same argument."""
    c = _edge_case(name)
    b32 = tol.ACCURATE_SPLIT_E32_FACTOR * c["e32"]
    b16 = tol.ACCURATE_F16_E16_FACTOR * c["e16"] + b32
    lib = _edge_volumes(name, layout, "library")[0].astype(np.float64)
    for route, bound in (("split", 2 * b32), ("f16", b16 + b32)):
        k = _edge_volumes(name, layout, route)[0]
        diff = np.abs(k - lib)
        diff[~c["mask"]] = 0.0
        worst = tuple(int(i) for i in np.unravel_index(int(diff.argmax()), diff.shape))
        print("%s %s %s: max |kernel - library| %.3e at (d,h,w) = %s, bound %.3e" % (name, layout, route, diff.max(),
                                                                                    worst, bound))
        assert diff.max() <= bound, "%s: (d,h,w) = %s" % (route, worst)


@pytest.mark.parametrize("route", ("split", "f16", "library"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(ar.EDGE_CASES))
def test_large_d_borders_and_right_volume_bit_identical(name, layout, route):
    """The literal float32 border recurrences and the right-volume copy on the GPU's own w >= d scores."""
    lcv, rcv, _flag = _edge_volumes(name, layout, route)
    want_l, want_r = ar.volumes_from_scores_by_column(lcv)
    helpers.assert_bits_strict(lcv, want_l, "%s %s %s: left volume" % (name, layout, route))
    helpers.assert_bits_strict(rcv, want_r, "%s %s %s: right volume" % (name, layout, route))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(ar.EDGE_CASES))
def test_large_d_layouts_give_the_same_bits(name, precision):
    a = _edge_volumes(name, "pixel_major", precision)
    b = _edge_volumes(name, "plane_major", precision)
    helpers.assert_bits_strict(a[0], b[0], "%s %s: left volume, pixel-major against plane-major" % (name, precision))
    helpers.assert_bits_strict(a[1], b[1], "%s %s: right volume, pixel-major against plane-major" % (name, precision))


# ---- (d): entries the call must not write ----------------------------------------------------------------------------
SENTINEL = 0x7fc0dead          # a NaN no kernel produces
PAD_D = (2, 33, 190, 513, 1022)


@functools.lru_cache(maxsize=None)
def _pad_case(D):
    """H = 2, W = D + 3: random halves of ordinary size (what is written matters here, not what it means)."""
    net = _pad_net()
    g = torch.Generator().manual_seed(D)
    aL = (torch.randn((2, D + 3, 384), generator=g) * 0.5).cuda()
    aR = (torch.randn((2, D + 3, 384), generator=g) * 0.5).cuda()
    return net, aL, aR


@functools.lru_cache(maxsize=None)
def _pad_net():
    return _make_net(112, 3, 11, 1.0)


def _sentinels(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


@pytest.mark.parametrize("route", ("split", "f16", "library"))
@pytest.mark.parametrize("D", PAD_D)
def test_pixel_major_pad_entries_are_not_written(D, route):
    """[H,W,Dp] volumes prefilled with a NaN pattern: afterwards every d >= D entry still holds it and no d < D entry
    does - by the kernel in either precision, and by the library route (accurate_scores_library + cost_volume_fill)."""
    import stereo_device as sd
    net, aL, aR = _pad_case(D)
    H, W = 2, D + 3
    Dp = sd.hwd_pitch(D)
    assert Dp - D == {2: 2, 33: 3, 190: 2, 513: 3, 1022: 2}[D]
    out = (_sentinels((H, W, Dp)), _sentinels((H, W, Dp)))
    if route == "library":
        sd.accurate_scores_library(net, aL, aR, D, out[0], out[1], True)
        sd.cost_volume_fill(out[0], out[1], D, True)
        torch.cuda.synchronize()
    else:
        _l, _r, flag = _launch(net, aL, aR, D, route, "pixel_major", out=out)
        assert flag == 0
    for what, vol in (("left", out[0]), ("right", out[1])):
        bits = vol.view(torch.int32)
        assert bool((bits[:, :, D:] == SENTINEL).all()), "%s volume: a pad entry was written" % what
        assert not bool((bits[:, :, :D] == SENTINEL).any()), "%s volume: a d < D entry was not written" % what
        assert bool(torch.isfinite(vol[:, :, :D]).all())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D", PAD_D)
def test_plane_major_guard_plane_is_intact(D, precision):
    """[D + 1, H, W] planes of the NaN pattern behind the pointer: the D planes are fully written, the guard plane is
    not touched."""
    net, aL, aR = _pad_case(D)
    H, W = 2, D + 3
    out = (_sentinels((D + 1, H, W)), _sentinels((D + 1, H, W)))
    _l, _r, flag = _launch(net, aL, aR, D, precision, "plane_major", out=out)
    assert flag == 0
    for what, vol in (("left", out[0]), ("right", out[1])):
        bits = vol.view(torch.int32)
        assert bool((bits[D] == SENTINEL).all()), "%s volume: the plane behind the last one was written" % what
        assert not bool((bits[:D] == SENTINEL).any()), "%s volume: an entry of the D planes was not written" % what


# ---- (e): through the matcher ----------------------------------------------------------------------------------------
def _poisoned_pairs():
    import synthetic
    H, W, D = 12, 48, 16
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=9)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    one_nan, one_ninf = dl.clone(), dl.clone()
    one_nan.view(H, W)[5, 20] = float("nan")
    one_ninf.view(H, W)[5, 20] = float("-inf")
    return D, dr, {"all_nan": torch.full_like(dl, float("nan")), "one_nan_pixel": one_nan,
                   "one_minus_inf_pixel": one_ninf}


@pytest.mark.parametrize("name", ("all_nan", "one_nan_pixel", "one_minus_inf_pixel"))
def test_matcher_repeats_a_poisoned_pair_on_the_library_route(name):
    """decision='kernel', default on_saturation, a left image that is all NaN (a constant image standardises to 0/0),
    has one NaN pixel, or one -inf pixel: the decision kernel raises its flag, the pair is repeated on the library
    route (the twin exists, the flag is read and reset) and the kept cost volumes are those of a decision='library'
    matcher bit for bit, NaN positions included.  The -inf pixel is the NaN case too: the tower's first layer makes
    +inf and -inf of it, the second adds them up (asserted below), so NaN reaches the decision stage.  The final map
    is not asserted: SGM over NaN is outside its contract."""
    import stereo_device as sd
    D, dr, lefts = _poisoned_pairs()
    dl = lefts[name]
    net = _make_net(112, 3, 11, 1.0)
    fl, _fr = net.features_pair_hwc(dl.reshape(dl.shape[0], dl.shape[1]).contiguous(),
                                    dr.reshape(dr.shape[0], dr.shape[1]).contiguous())
    assert bool(torch.isnan(fl).any()), "the tower handed on no NaN: this is another case than the docstring says"
    want = {}
    sd.StereoMatcher(net, decision="library").match(dl, dr, D, keep=want)
    m = sd.StereoMatcher(net, decision="kernel")
    assert m.on_saturation == "fallback" and m._library_twin is None
    keep = {}
    m.match(dl, dr, D, keep=keep)
    torch.cuda.synchronize()
    assert m._library_twin is not None and m._library_twin.decision == "library", "the fallback did not fire"
    assert not m.features_saturated()                        # read and reset by the fallback
    assert bool(torch.isnan(want["cv"][0]).any()), "the library route hands out the network's NaN"
    for i, side in enumerate(("left", "right")):
        helpers.assert_bits_strict(keep["cv"][i].cpu().numpy(), want["cv"][i].cpu().numpy(),
                                   "%s: kept %s cost volume against decision='library'" % (name, side))


def test_matcher_raises_on_a_nan_pair():
    import stereo_device as sd
    D, dr, lefts = _poisoned_pairs()
    net = _make_net(112, 3, 11, 1.0)
    with pytest.raises(RuntimeError, match="decision kernel"):
        sd.StereoMatcher(net, decision="kernel", on_saturation="raise").match(lefts["all_nan"], dr, D)
