"""GPU: more than 512 disparities (full-resolution Middlebury declares up to 760; the kernels serve up to 1024), bit for
bit against the CPU oracle, which has no disparity limit: the SGM passes with three and four 256-disparity groups per
lane, the pixel-major cost volume, a default StereoMatcher on both pixel-major aggregation kernels, and match.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits, assert_bits_strict
import tolerances as tol

pytestmark = pytest.mark.gpu

SGM_HP = (2.3, 55.9, 4, 8, 0.08)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def env(net_layers):
    import _hipabi as hip
    hip.require_device()
    import oracle
    import stereo_device
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    return dict(hip=hip, o=oracle, sd=stereo_device, net=net)


# ---- SGM, one pass at a time ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D", [(7, 515, 513), (19, 650, 640), (5, 770, 768), (11, 805, 800), (21, 1026, 1024),
                                   (4, 1100, 1024)])
def test_sgm_passes_large_d_match_the_oracle(env, H, W, D):
    """Every direction and side through mccnn_sgm_pass and through mccnn_sgm_flags + mccnn_sgm_pass_flagged, with +inf
    costs scattered through the volume: full groups (768, 1024), masked tails (513, 640, 800), scanlines shorter and
    longer than two blocks of steps in flight."""
    o, sd = env["o"], env["sd"]
    import synthetic
    rng = np.random.default_rng(D + H)
    L, R, _, _, _ = synthetic.make_pair(H, W, 16, seed=D)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    v = (rng.random((D, H, W), dtype=np.float32) * 4 - 2).astype(np.float32)
    v[rng.random((D, H, W)) < 0.02] = np.inf
    v[0][np.isinf(v).all(axis=0)] = 1.0
    p1, p2, q1, q2, thr = (sd._f32(x) for x in SGM_HP)
    scratch = sd.sgm_scratch(H, W, D, l.device)
    for r_ in sd.SGM_DIRECTIONS:
        flags = sd.sgm_flag_planes(l, r, D, SGM_HP[4])[sd.SGM_DIRECTIONS.index(r_)]
        for side, choice in ((env["hip"].MCCNN_SIDE_LEFT, "L"), (env["hip"].MCCNN_SIDE_RIGHT, "R")):
            want = o.semi_global_matching(L, R, v.copy(), r_, *SGM_HP, choice)
            assert np.isinf(want).any()
            a = sd.dhw_to_hwd(dev(v))
            sd.sgm_pass_hwd(l, r, [a], [side], D, r_, p1, p2, q1, q2, thr, scratch)
            b = sd.dhw_to_hwd(dev(v))
            sd.sgm_pass_flagged_hwd([b], [side], D, r_, p1, p2, q1, q2, flags)
            what = "D=%d r=%s side %s" % (D, r_, choice)
            assert_bits(sd.hwd_to_dhw(a, D).cpu().numpy(), want, what + ", mccnn_sgm_pass")
            assert_bits(sd.hwd_to_dhw(b, D).cpu().numpy(), want, what + ", mccnn_sgm_pass_flagged")


def test_sgm_two_volume_launch_large_d(env):
    """One launch advancing both volumes of a pair (n_jobs = 2) at D = 800: the oracle's SGM_average of both."""
    o, sd = env["o"], env["sd"]
    import synthetic
    H, W, D = 9, 830, 800
    rng = np.random.default_rng(3)
    L, R, _, _, _ = synthetic.make_pair(H, W, 16, seed=4)
    vl = (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    vr = (-rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    want = o.SGM_average(vl.copy(), vr.copy(), L, R, *SGM_HP, 1.5)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    a, b = sd.dhw_to_hwd(dev(vl)), sd.dhw_to_hwd(dev(vr))
    sd.sgm_average_hwd(l, r, [a, b], [0, 1], D, *SGM_HP, 1.5, sd.sgm_scratch(H, W, D, l.device))
    assert_bits(sd.hwd_to_dhw(a, D).cpu().numpy(), want[0], "SGM_average D=800 (left)")
    assert_bits(sd.hwd_to_dhw(b, D).cpu().numpy(), want[1], "SGM_average D=800 (right)")


def test_sgm_refuses_more_than_1024_disparities(env):
    sd, hip = env["sd"], env["hip"]
    H, W, D = 2, 1040, 1025
    l = torch.zeros((H, W), device="cuda")
    v = torch.zeros((H, W, sd.hwd_pitch(D)), device="cuda")
    with pytest.raises(RuntimeError, match="1024"):
        sd.sgm_pass_hwd(l, l, [v], [hip.MCCNN_SIDE_LEFT], D, (0, 1), 1.0, 2.0, 4.0, 8.0, 0.08,
                        sd.sgm_scratch(H, W, D, l.device))


# ---- pixel-major cost volume ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D", [(3, 700, 640), (2, 1030, 1024)])
def test_cost_volume_hwd_large_d_matches_the_oracle(env, H, W, D):
    """Exact mode bit for bit against oracle.compute_cost_volume (border fill included); the matrix-core mode within
    tolerances.COST_VOLUME_MFMA_ABS of it on unit feature vectors."""
    o, sd, hip = env["o"], env["sd"], env["hip"]
    g = torch.Generator(device="cuda").manual_seed(D)
    fl = torch.nn.functional.normalize(torch.randn((H, W, 64), device="cuda", generator=g), dim=-1)
    fr = torch.nn.functional.normalize(torch.randn((H, W, 64), device="cuda", generator=g), dim=-1)
    wl, wr = o.compute_cost_volume(fl.cpu().numpy(), fr.cpu().numpy(), D)
    lh, rh = sd.cost_volume_hwd(fl, fr, D)
    assert_bits(sd.hwd_to_dhw(lh, D).cpu().numpy(), wl, "exact, left D=%d" % D)
    assert_bits(sd.hwd_to_dhw(rh, D).cpu().numpy(), wr, "exact, right D=%d" % D)
    lm, rm = sd.cost_volume_hwd(fl, fr, D, mode=hip.MCCNN_CV_MFMA)
    for got, want, name in ((lm, wl, "left"), (rm, wr, "right")):
        err = np.abs(sd.hwd_to_dhw(got, D).cpu().numpy().astype(np.float64) - want.astype(np.float64))
        assert float(err.max()) <= tol.COST_VOLUME_MFMA_ABS, "matrix cores, %s D=%d: %g" % (name, D, float(err.max()))


# ---- a default StereoMatcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,progs", [(12, 1100, 640, True), (12, 1100, 1024, True), (8, 2400, 800, False)],
                         ids=["prog_640", "prog_1024", "cbca_hwd_800"])
def test_default_matcher_large_d_matches_the_oracle(env, H, W, D, progs):
    """match() and match_graph() of a default StereoMatcher against oracle.match_from_features fed the GPU's own
    features, on row windows of full-resolution widths: W <= 2180 runs the program-driven assembly aggregation, wider
    rows cbca_hwd_kernel."""
    o, sd, net = env["o"], env["sd"], env["net"]
    import synthetic
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=D + W)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    fl, fr = (t.cpu().numpy() for t in net.features_pair_hwc_split(l, r))
    assert not net.split_saturated(True)
    want = o.match_from_features(L, R, fl, fr, D)
    m = sd.StereoMatcher(net)
    assert m.pixel_major() and m.features == "split_f16"
    ws = m.workspace(H, W, D)
    assert (ws["progs"] is not None) == progs
    assert_bits_strict(m.match(l, r, D).cpu().numpy(), want, "match() %dx%dx%d" % (W, H, D))
    assert_bits_strict(m.match_graph(l, r, D).cpu().numpy(), want, "match_graph() %dx%dx%d" % (W, H, D))


# ---- match.py -----------------------------------------------------------------------------------------------------------
def test_match_cli_large_ndisp_equals_the_matcher(env, tmp_path):
    """match.py on PNG files whose calib.txt declares ndisp = 760 (Vintage's value): the PFM it writes equals
    StereoMatcher's map of the same decoded, standardised images."""
    from PIL import Image
    import synthetic
    import util
    sd, net = env["sd"], env["net"]
    H, W, D = 14, 1000, 760
    pair = tmp_path / "data" / "trainingF" / "Vintage"
    os.makedirs(str(pair))
    L, R, _, _, _ = synthetic.make_pair(H, W, D, seed=7)
    for name, img in (("im0.png", L), ("im1.png", R)):
        g = img[:, :, 0]
        g8 = np.clip((g - g.min()) / (g.max() - g.min()) * 255.0, 0, 255).astype(np.uint8)
        Image.fromarray(g8, mode="L").save(str(pair / name))
    (pair / "calib.txt").write_text("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                                    "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n"
                                    % (W, H, D, D))
    lst = tmp_path / "list.txt"
    lst.write_text("%s/im0.png\n" % pair)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0",
           "--list_file", str(lst), "--resume", os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"),
           "--data_dir", str(tmp_path / "data"), "--save_dir", str(out), "-t", "big", "-s", "0", "-e", "0"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    disp = util.readPfm(str(out / "submit_big" / "trainingF" / "Vintage" / "disp0MCCNN.pfm"))
    disp = np.asarray(disp[0] if isinstance(disp, tuple) else disp, np.float32).reshape(H, W)
    views = []
    for name in ("im0.png", "im1.png"):
        g = util.read_gray(str(pair / name)).astype(np.float32)
        views.append(dev((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1))))
    want = sd.StereoMatcher(net).match(views[0], views[1], D).cpu().numpy()
    assert_bits_strict(disp, want, "match.py PFM vs StereoMatcher, ndisp=%d" % D)
