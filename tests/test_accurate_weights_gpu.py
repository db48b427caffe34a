"""GPU: the accurate network's decision stage on the weights a trained network may have - the families of
tests/accurate_reference.py (layers of different magnitude, outliers, heavy tails, zeros, tiny, huge and non-finite
weights; their premises are tests/test_accurate_weights_cpu.py's) - and the accurate network's training step on the
device.  Bounds are the project's own (src/tolerances.py), multiples of E32 and E16 computed on the same inputs by
ar.yardsticks, never from the kernel.  Every w >= d voxel takes part; each device step runs once (lru_cache)."""
import functools
import math

import numpy as np
import pytest
import torch

import accurate_reference as ar
import helpers
import tolerances as tol

pytestmark = pytest.mark.gpu

SEED = 11
# name -> (H, W, D, feature maps, fc layers, patch): D crosses one 32-disparity block and W % 4 != 0; the KITTI shape
CASES = {"5x67x33": (5, 67, 33, 112, 3, 11), "kitti_6x70x40": (6, 70, 40, 64, 4, 9)}
LAYOUTS = ("pixel_major", "plane_major")
SCORED = [(case, name) for case, v in CASES.items() for name in ar.score_families(v[4])]
BORDER_FAMILIES = ("gap_2^12", "tiny_1e-34")


def _new_net(C, n_fc, patch, fc=None, device="cuda"):
    """The seeded glorot network, its decision network replaced by the lists `fc` where given."""
    from model import ACCURATE_NET
    net = ACCURATE_NET(None, input_patch_size=patch, num_conv_layers=(patch - 1) // 2, num_conv_feature_maps=C,
                       num_fc_layers=n_fc, batch_size=1, device=device, seed=SEED)
    if fc is not None:
        net.fc_weights = [w.clone().to(device) for w, _b in fc]
        net.fc_biases = [b.clone().to(device) for _w, b in fc]
    return net


@functools.lru_cache(maxsize=None)
def _case(case):
    """The tower outputs of a smooth pair: the decision stage's inputs, the same for every family (the tower is glorot's)."""
    H, W, D, C, n_fc, patch = CASES[case]
    net = _new_net(C, n_fc, patch)
    L, R = (t.cuda() for t in helpers.smooth_pair(H, W, seed=H + W))
    fl, fr = net.features_pair_hwc(L, R)
    torch.cuda.synchronize()
    return dict(fl=fl, fr=fr, fl_cpu=fl.cpu(), fr_cpu=fr.cpu(), mask=ar.valid_mask(D, H, W))


@functools.lru_cache(maxsize=None)
def _family(case, name):
    """The family's network on the device and the yardsticks on the case's inputs, with the premises that make a pass
    mean something: ordered yardsticks, float64 pre-activations below half the operand limit (the flag must be 0)."""
    H, W, D, C, n_fc, patch = CASES[case]
    c = _case(case)
    _conv, fc = ar.weight_family(name, C, n_fc, SEED, inputs=(c["fl_cpu"], c["fr_cpu"], D), patch=patch)
    s64, e32, e16 = ar.yardsticks(fc, c["fl_cpu"], c["fr_cpu"], D)
    assert e32 > 0.0 and e16 > e32
    first, hidden = ar.hidden_preactivation_max(fc, c["fl_cpu"], c["fr_cpu"], D)
    assert first < ar.PREMISE_LIMIT and hidden < ar.PREMISE_LIMIT, (name, first, hidden)
    assert int(c["mask"].sum()) == H * sum(W - d for d in range(D))
    return dict(net=_new_net(C, n_fc, patch, fc), fc=fc, s64=s64, e32=e32, e16=e16)


@functools.lru_cache(maxsize=None)
def _volumes(case, name, layout, decision, precision):
    """(lcv, rcv) float32 [D,H,W] on the host + the saturation flag, from ONE call of cost_volume_accurate."""
    import _hipabi as hip
    import stereo_device as sd
    D = CASES[case][2]
    c, f = _case(case), _family(case, name)
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    pm = layout == "pixel_major"
    mode = hip.MCCNN_CV_EXACT if precision == "split" else hip.MCCNN_CV_MFMA
    lcv, rcv = sd.cost_volume_accurate(f["net"], c["fl"], c["fr"], D, mode=mode, decision=decision, pixel_major=pm,
                                       sat_flag=flag if decision == "kernel" else None)
    torch.cuda.synchronize()
    if pm:
        lcv, rcv = sd.hwd_to_dhw(lcv, D), sd.hwd_to_dhw(rcv, D)
    return lcv.cpu().numpy(), rcv.cpu().numpy(), int(flag.item())


def _score_error(case, name, lcv):
    return float(np.abs(-lcv.astype(np.float64) - _family(case, name)["s64"])[_case(case)["mask"]].max())


def _f16_bound(f):
    return tol.ACCURATE_F16_E16_FACTOR * f["e16"] + tol.ACCURATE_SPLIT_E32_FACTOR * f["e32"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case,name", SCORED)
def test_scores_split_precision(case, name, layout):
    """Split operands: every w >= d score within 4 x E32 of float64, the flag down, on every family."""
    f = _family(case, name)
    lcv, _rcv, flag = _volumes(case, name, layout, "kernel", "split")
    err = _score_error(case, name, lcv)
    print("FAMILY %s %s %s: split kernel err %.3e = %.2f x E32 (E32 %.3e)" % (case, name, layout, err, err / f["e32"],
                                                                            f["e32"]))
    assert flag == 0
    assert np.isfinite(lcv).all()
    assert err <= tol.ACCURATE_SPLIT_E32_FACTOR * f["e32"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case,name", SCORED)
def test_scores_f16_precision(case, name, layout):
    """One f16 product per multiply: within 2 x E16 + 4 x E32, the flag down, on every family."""
    f = _family(case, name)
    lcv, _rcv, flag = _volumes(case, name, layout, "kernel", "f16")
    err = _score_error(case, name, lcv)
    print("FAMILY %s %s %s: f16 kernel err %.3e = %.2f of its bound (E16 %.3e)" % (case, name, layout, err,
                                                                                 err / _f16_bound(f), f["e16"]))
    assert flag == 0
    assert err <= _f16_bound(f)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case,name", SCORED)
def test_kernel_and_library_routes_agree(case, name, layout):
    """The library route is float32 throughout and does not care about the family; the two routes agree."""
    f, mask = _family(case, name), _case(case)["mask"]
    k = _volumes(case, name, layout, "kernel", "split")[0]
    l = _volumes(case, name, layout, "library", "split")[0]
    lib_err = _score_error(case, name, l)
    print("FAMILY %s %s %s: library err %.3e = %.2f x E32" % (case, name, layout, lib_err, lib_err / f["e32"]))
    assert lib_err <= tol.ACCURATE_SPLIT_E32_FACTOR * f["e32"]
    assert float(np.abs(k.astype(np.float64) - l)[mask].max()) <= tol.ACCURATE_SPLIT_E32_FACTOR * f["e32"]


@pytest.mark.parametrize("case", list(CASES))
def test_no_family_is_routed_away_from_the_kernel(case):
    """decision='auto' keeps every scored family - laplace and sparse_95 among them - on the kernel, without a
    warning; the equalised operands are cached per weight set."""
    import warnings
    import _hipabi as hip
    import stereo_device as sd
    _H, W, D = CASES[case][:3]
    for name in ar.score_families(CASES[case][4]):
        net = _family(case, name)["net"]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert sd.StereoMatcher(net, decision="auto").decision_route(W, D) == "kernel", name
        assert net.decision_operands(hip.MCCNN_CV_EXACT) is net.decision_operands(hip.MCCNN_CV_EXACT)


@pytest.mark.parametrize("decision", ("kernel", "library"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", BORDER_FAMILIES)
@pytest.mark.parametrize("case", list(CASES))
def test_borders_and_right_volume_bit_identical(case, name, layout, decision):
    lcv, rcv, _flag = _volumes(case, name, layout, decision, "split")
    want_l, want_r = ar.volumes_from_scores(lcv)
    helpers.assert_bits_strict(lcv, want_l, "%s %s %s %s: left volume" % (case, name, layout, decision))
    helpers.assert_bits_strict(rcv, want_r, "%s %s %s %s: right volume" % (case, name, layout, decision))


@pytest.mark.parametrize("case", list(CASES))
def test_glorot_operands_are_the_unequalised_ones(case):
    """Layers that already share a binade are packed as they are: c_k = 1, the packed bytes of the plain layers."""
    import _hipabi as hip
    import stereo_device as sd
    net = _family(case, "glorot")["net"]
    assert net.decision_layers()[4] == [0] * (net.num_fc_layers - 1)
    packed, scale, biases, w_final, b_final = net.decision_operands(hip.MCCNN_CV_EXACT)
    plain, plain_scale = sd.decision_pack(torch.stack(net.fc_weights[1:-1]), net.num_fc_layers, hip.MCCNN_CV_EXACT)
    assert scale == plain_scale and torch.equal(packed, plain)
    assert torch.equal(biases, torch.stack(net.fc_biases[1:-1])) and torch.equal(w_final, net.fc_weights[-1].reshape(-1))
    assert b_final == float(net.fc_biases[-1][0])


@pytest.mark.parametrize("precision", ("split", "f16"))
def test_huge_weights_raise_the_flag(precision):
    """huge_1e30: finite weights the operands hold, activations they do not - the flag goes up (the pair then goes to
    the library route); the stored volumes are finite."""
    import _hipabi as hip
    import stereo_device as sd
    case = "5x67x33"
    H, W, D, C, n_fc, patch = CASES[case]
    c = _case(case)
    _conv, fc = ar.weight_family("huge_1e30", C, n_fc, SEED)
    net = _new_net(C, n_fc, patch, fc)
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    mode = hip.MCCNN_CV_EXACT if precision == "split" else hip.MCCNN_CV_MFMA
    lcv, _rcv = sd.cost_volume_accurate(net, c["fl"], c["fr"], D, mode=mode, decision="kernel", sat_flag=flag)
    assert int(flag.item()) == 1
    assert bool(torch.isfinite(lcv[:, :, :D]).all())


@pytest.mark.parametrize("name", ar.NONFINITE_FAMILIES)
def test_non_finite_weights_are_refused(name):
    """+inf, -inf or NaN among the hidden weights: the kernel route refuses before anything is launched, naming the
    layer (the earlier rule packed them with scale 1, clamped: a finite wrong score and no flag); the library route
    returns what the network computes."""
    import _hipabi as hip
    import stereo_device as sd
    case = "5x67x33"
    H, W, D, C, n_fc, patch = CASES[case]
    c = _case(case)
    _conv, fc = ar.weight_family(name, C, n_fc, SEED)
    layer = [k + 1 for k, (w, _b) in enumerate(fc) if not bool(torch.isfinite(w).all())][0]
    net = _new_net(C, n_fc, patch, fc)
    out = tuple(torch.full((H, W, sd.hwd_pitch(D)), 5.0, device="cuda") for _ in range(2))
    for mode in (hip.MCCNN_CV_EXACT, hip.MCCNN_CV_MFMA):
        with pytest.raises(hip.MccnnHipError, match="fc%d" % layer):
            sd.cost_volume_accurate(net, c["fl"], c["fr"], D, mode=mode, decision="kernel", out=out)
    with pytest.raises(hip.MccnnHipError, match="finite"):
        sd.decision_pack(torch.stack(net.fc_weights[1:-1]), n_fc, hip.MCCNN_CV_EXACT)
    torch.cuda.synchronize()
    assert bool((out[0] == 5.0).all()) and bool((out[1] == 5.0).all())
    lcv, _rcv = sd.cost_volume_accurate(net, c["fl"], c["fr"], D, decision="library")
    want = ar.scores(fc, c["fl_cpu"], c["fr_cpu"], D, torch.float32)
    got = -sd.hwd_to_dhw(lcv, D).cpu().numpy().astype(np.float64)
    m = c["mask"]
    # (inf * relu(x) is NaN where x <= 0 and inf where x > 0: a voxel whose x is within rounding of 0 may differ between
    # two float32 evaluations, so the NaN pattern is compared as a whole and the values where both are numbers)
    assert not np.isfinite(want[m]).all(), "the family was meant to reach the scores"
    assert bool(np.isnan(got[m]).any()) == bool(np.isnan(want[m]).any())
    ok = m & np.isfinite(want) & np.isfinite(got)
    assert not ok.any() or np.abs(got[ok] - want[ok]).max() <= 1e-6


def test_whole_pair_with_a_layer_gap():
    """A StereoMatcher pair on gap_2^12 weights, decision='kernel' and 'library': the kept cost volumes meet the bound,
    no fallback happened, and the graph replay is the eager map bit for bit."""
    import stereo_device as sd
    import synthetic
    H, W, D, C, n_fc, patch = 12, 48, 16, 112, 3, 11
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=5)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    base = _new_net(C, n_fc, patch)
    fl, fr = base.features_pair_hwc(dl[:, :, 0].contiguous(), dr[:, :, 0].contiguous())
    _conv, fc = ar.weight_family("gap_2^12", C, n_fc, SEED)
    s64, e32, _e16 = ar.yardsticks(fc, fl.cpu(), fr.cpu(), D)
    first, hidden = ar.hidden_preactivation_max(fc, fl.cpu(), fr.cpu(), D)
    assert e32 > 0.0 and first < ar.PREMISE_LIMIT and hidden < ar.PREMISE_LIMIT
    mask = ar.valid_mask(D, H, W)
    net = _new_net(C, n_fc, patch, fc)
    m = sd.StereoMatcher(net, decision="kernel")
    keep = {}
    out = m.match(dl, dr, D, keep=keep)
    torch.cuda.synchronize()
    assert m._library_twin is None and m.saturation_checked() and not m.features_saturated()
    cv_l = keep["cv"][0].cpu().numpy()
    err = float(np.abs(-cv_l.astype(np.float64) - s64)[mask].max())
    print("FAMILY whole pair gap_2^12: kept volume err %.3e = %.2f x E32" % (err, err / e32))
    assert err <= tol.ACCURATE_SPLIT_E32_FACTOR * e32
    want_l, want_r = ar.volumes_from_scores(cv_l)
    helpers.assert_bits_strict(cv_l, want_l, "kept left volume")
    helpers.assert_bits_strict(keep["cv"][1].cpu().numpy(), want_r, "kept right volume")
    eager = m.match(dl, dr, D).cpu().numpy()
    helpers.assert_bits_strict(eager, out.cpu().numpy(), "match() without keep")
    helpers.assert_bits_strict(m.match_graph(dl, dr, D).cpu().numpy(), eager, "match_graph against match")
    assert m._library_twin is None
    ml = sd.StereoMatcher(net, decision="library")
    keep_l = {}
    ml.match(dl, dr, D, keep=keep_l)
    lib = keep_l["cv"][0].cpu().numpy()
    lib_err = float(np.abs(-lib.astype(np.float64) - s64)[mask].max())
    assert lib_err <= tol.ACCURATE_SPLIT_E32_FACTOR * e32
    assert float(np.abs(lib.astype(np.float64) - cv_l)[mask].max()) <= tol.ACCURATE_SPLIT_E32_FACTOR * e32


@pytest.mark.parametrize("bad", (float("inf"), float("nan"), float("-inf"), 0.0, 2.0 ** 120))
def test_entry_points_require_a_finite_weight_scale(bad):
    """mccnn_decision_pack and both mccnn_cost_volume_accurate* return MCCNN_E_INVALID for a weight_scale that is inf,
    NaN or outside the range in which scale * 256 is a normal float32, name the argument, and touch no output."""
    import _hipabi as hip
    import stereo_device as sd
    lib = hip.load()
    H, W, D = 4, 20, 8
    net = _new_net(112, 3, 11)
    w = torch.stack(net.fc_weights[1:-1]).contiguous()
    nbytes = int(lib.mccnn_decision_pack_bytes(3, 384, hip.MCCNN_CV_EXACT))
    packed = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda")
    rc = lib.mccnn_decision_pack(hip.ptr(w), 3, 384, bad, hip.MCCNN_CV_EXACT, hip.ptr(packed), hip.stream())
    assert rc == hip.MCCNN_E_INVALID and b"weight_scale" in lib.mccnn_last_error_string()
    torch.cuda.synchronize()
    assert bool((packed == 0x5a).all())
    good, _scale, biases, w_final, b_final = net.decision_operands(hip.MCCNN_CV_EXACT)
    a = torch.rand((H, W, 384), device="cuda")
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for fn, shape in ((lib.mccnn_cost_volume_accurate_hwd, (H, W, sd.hwd_pitch(D))),
                      (lib.mccnn_cost_volume_accurate, (D, H, W))):
        vols = tuple(torch.full(shape, 5.0, device="cuda") for _ in range(2))
        rc = fn(hip.ptr(a), hip.ptr(a), H, W, 112, 384, 3, D, hip.ptr(good), hip.ptr(biases), hip.ptr(w_final), b_final,
                bad, hip.ptr(vols[0]), hip.ptr(vols[1]), hip.MCCNN_CV_EXACT, hip.ptr(flag), hip.stream())
        assert rc == hip.MCCNN_E_INVALID and b"weight_scale" in lib.mccnn_last_error_string()
        torch.cuda.synchronize()
        assert bool((vols[0] == 5.0).all()) and bool((vols[1] == 5.0).all()) and int(flag.item()) == 0


# ---- the accurate network's training step on the device ---------------------------------------------------------------
def two_bce_steps(device, B=16, lr=0.05, beta=0.9):
    """Two Trainer.step calls of ACCURATE_NET(112 maps, 3 fc) under BCE on `device` against a float64 CPU evaluation
    written out here: three weight-shared towers (ReLU after every VALID 3x3 convolution), the decision network on
    [fL ; fR], loss = (sum -log s+  +  sum -log(1 - s-)) / 2B, momentum SGD (accum = beta * accum + grad;
    var -= lr * accum).  Returns (device losses, float64 losses, worst |updated tensor - float64|, largest move)."""
    import torch.nn.functional as F
    import train
    from model import ACCURATE_NET
    rng = np.random.default_rng(7)
    base = rng.standard_normal((B, 11, 11, 1)).astype(np.float32)
    batches = [[base + 0.1 * rng.standard_normal(base.shape).astype(np.float32),
                base + 0.1 * rng.standard_normal(base.shape).astype(np.float32),
                rng.standard_normal(base.shape).astype(np.float32)] for _ in range(2)]
    net = ACCURATE_NET(None, batch_size=B, device=device, seed=2)
    conv, fc = ar.net_lists(net)
    t = train.Trainer(net, lr, beta, 0.2)
    got_losses = [t.step(*b) for b in batches]
    now = [p for k in range(len(conv)) for p in (net.weights[k], net.biases[k])] + \
          [p for k in range(len(fc)) for p in (net.fc_weights[k], net.fc_biases[k])]

    params = [x.clone().double().requires_grad_(True) for pair in conv + fc for x in pair]
    start = [p.detach().clone() for p in params]
    n_conv = len(conv)
    acc = [torch.zeros_like(p) for p in params]
    want_losses = []
    for batch in batches:
        feats = []
        for patches in batch:
            x = torch.tensor(patches.astype(np.float64)).permute(0, 3, 1, 2)
            for k in range(n_conv):
                x = torch.relu(F.conv2d(x, params[2 * k], params[2 * k + 1]))
            feats.append(x.reshape(B, -1))

        def score(a, b):
            x = torch.cat((a, b), -1)
            for k in range(len(fc)):
                x = x @ params[2 * (n_conv + k)].t() + params[2 * (n_conv + k) + 1]
                if k < len(fc) - 1:
                    x = torch.relu(x)
            return torch.sigmoid(x[:, 0])

        loss = (-torch.log(score(feats[0], feats[1])).sum() - torch.log(1 - score(feats[0], feats[2])).sum()) / (2 * B)
        want_losses.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            for p, a, g in zip(params, acc, grads):
                a.mul_(beta).add_(g)
                p.sub_(lr * a)
    worst = max(float((p.detach().double().cpu() - p64.detach()).abs().max()) for p, p64 in zip(now, params))
    moved = max(float((p64.detach() - s).abs().max()) for p64, s in zip(params, start))
    return got_losses, want_losses, worst, moved


def test_two_bce_steps_match_float64():
    """Backward through the 112-map library convolutions and the fc stack on the device: both losses and all eighteen
    updated tensors within 1e-5 of float64; the steps moved the weights; the BCE is away from log 2 (scores away from
    1/2), so the gradient is not the degenerate one of an undecided network."""
    got, want, worst, moved = two_bce_steps("cuda")
    print("two BCE steps: losses %s (float64 %s), worst tensor error %.3e, largest move %.3e" % (got, want, worst, moved))
    assert all(abs(w - math.log(2.0)) > 1e-4 for w in want), want
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-5, (got, want)
    assert moved > 1e-4, "the steps did not move the weights"
    assert worst <= 1e-5, "updated tensors differ from the float64 evaluation by %g" % worst


def _trainer_and_batch(B=16):
    import train
    from model import ACCURATE_NET
    rng = np.random.default_rng(3)
    batch = [rng.standard_normal((B, 11, 11, 1)).astype(np.float32) for _ in range(3)]
    net = ACCURATE_NET(None, batch_size=B, device="cuda", seed=4)
    return net, train.Trainer(net, 0.05, 0.9, 0.2), batch


def _assert_repacked(net, before, snapshot, modes):
    import stereo_device as sd
    for mode in modes:
        after = net.decision_operands(mode)
        assert after is not before[mode]
        assert net.decision_operands(mode) is after
        w, b, w_final, b_final, _exps = net.decision_layers()
        fresh, fresh_scale = sd.decision_pack(w, net.num_fc_layers, mode)
        assert after[1] == fresh_scale and torch.equal(after[0], fresh)
        assert torch.equal(after[2], b) and torch.equal(after[3], w_final) and after[4] == float(b_final[0])
        assert not torch.equal(after[0], snapshot[mode][0]) and not torch.equal(after[2], snapshot[mode][1])


def test_decision_cache_repacks_after_a_step_and_after_load_state(tmp_path):
    """net.decision_operands(mode) is one object until a weight tensor changes; after an optimiser step, and after
    Trainer.load_state's copy_ under no_grad, it is a new one, bit-equal to a fresh pack of the new weights and
    different from the snapshot taken before."""
    import _hipabi as hip
    import tf_checkpoint
    modes = (hip.MCCNN_CV_EXACT, hip.MCCNN_CV_MFMA)
    net, t, batch = _trainer_and_batch()
    start_path = str(tmp_path / "start.npz")
    tf_checkpoint.save_npz(start_path, net.get_layers(), net.get_fc_layers())
    before = {mode: net.decision_operands(mode) for mode in modes[:1]}
    assert net.decision_operands(modes[0]) is before[modes[0]]
    before[modes[1]] = net.decision_operands(modes[1])       # (one mode is cached at a time)
    assert net.decision_operands(modes[1]) is before[modes[1]]
    snapshot = {mode: (before[mode][0].clone(), before[mode][2].clone()) for mode in modes}
    t.step(*batch)
    _assert_repacked(net, before, snapshot, modes)
    stepped = {mode: net.decision_operands(mode) for mode in modes[1:]}
    stepped_snapshot = {mode: (stepped[mode][0].clone(), stepped[mode][2].clone()) for mode in modes[1:]}
    t.load_state(start_path)                                 # back to the first weights, through copy_
    _assert_repacked(net, stepped, stepped_snapshot, modes[1:])
    back = net.decision_operands(modes[1])
    assert torch.equal(back[0], snapshot[modes[1]][0]) and torch.equal(back[2], snapshot[modes[1]][1])


@pytest.mark.parametrize("how", ("eager", "graph"))
def test_one_matcher_across_an_optimiser_step(how):
    """train.py --val_error keeps ONE StereoMatcher over all epochs: its map after a step is, bit for bit, the map of
    a matcher built on the stepped network, and not the map before the step - eager, and through match_graph, whose
    captured graph holds the address of the packed operands of the weights it was captured with."""
    import stereo_device as sd
    import synthetic
    H, W, D = 12, 48, 16
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=5)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    net, t, batch = _trainer_and_batch()
    m = sd.StereoMatcher(net, decision="kernel")
    run = (lambda x: x.match(dl, dr, D)) if how == "eager" else (lambda x: x.match_graph(dl, dr, D))
    with torch.no_grad():
        before = run(m).cpu().numpy()
        helpers.assert_bits_strict(run(m).cpu().numpy(), before, "%s: the same weights twice" % how)
    t.step(*batch)
    with torch.no_grad():
        after = run(m).cpu().numpy()
        fresh = sd.StereoMatcher(net, decision="kernel").match(dl, dr, D).cpu().numpy()
    assert m._library_twin is None
    helpers.assert_bits_strict(after, fresh, "%s: the kept matcher on the stepped network" % how)
    assert not helpers.bits_strict(after, before), "the step did not move the map"
