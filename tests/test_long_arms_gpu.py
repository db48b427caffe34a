"""GPU: cbca_distance 15 to 32 on the pixel-major path - mccnn_cbca_iter_hwd_long(_pair) through the C ABI against the
CPU oracle and against the plane-major reference-order kernel, and the whole pair (StereoMatcher, match_graph,
match.py with and without --pipeline) on the route it selects.  Every comparison is bit for bit.

The conditions that keep a comparison from passing vacuously (arms really reach L - 1, a good share of the pixels has
an arm no kernel for L <= 14 serves) are asserted on oracle.cross_arms of the very inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits

pytestmark = pytest.mark.gpu

TAU = 0.02


@pytest.fixture(scope="module")
def sd():
    import _hipabi
    _hipabi.require_device()
    import stereo_device
    return stereo_device


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blocks(H, W):
    """40 x 40 blocks of the grey levels 0 and 1, [H,W,1] float32: inside a block every arm runs to the block's edge
    or to the distance limit."""
    y, x = np.indices((H, W))
    return (((x // 40 + y // 40) % 2).astype(np.float32))[:, :, None]


def long_arm_share(img, dist):
    """(largest arm, share of the pixels with an arm of 14 or more) by the CPU oracle."""
    import oracle as o
    arms = o.cross_arms(img, TAU, dist)[0]
    return int(arms.max()), float((arms.max(axis=2) >= 14).mean())


def _agg(sd, vol_dhw, image, dist, n):
    """n reference-order iterations through sd.cbca_hwd (which picks the entry point by distance); numpy in and out."""
    v = dev(vol_dhw)
    D = v.shape[0]
    sup = sd.cross_arms(dev(image[:, :, 0]), TAU, dist)
    hv = sd.dhw_to_hwd(v)
    res, _ = sd.cbca_hwd(hv, torch.full_like(hv, float("nan")), sup, D, n, dist)
    return sd.hwd_to_dhw(res, D).cpu().numpy()


def _long(sd, vol_dhw, sup, dist, n=1):
    """n iterations through mccnn_cbca_iter_hwd_long itself, whatever the distance; device [D,H,W] in and out."""
    import _hipabi as hip
    D, H, W = vol_dhw.shape
    src = sd.dhw_to_hwd(vol_dhw)
    dst = torch.full_like(src, float("nan"))
    for _ in range(n):
        hip.check(hip.load().mccnn_cbca_iter_hwd_long(hip.ptr(src), hip.ptr(dst), hip.ptr(sup), D, H, W, dist, hip.stream()),
                  "mccnn_cbca_iter_hwd_long")
        src, dst = dst, src
    return sd.hwd_to_dhw(src, D)


# ---- 1. oracle, ragged shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D", [(70, 75, 5), (40, 131, 64), (24, 97, 200), (24, 70, 192), (10, 40, 150), (12, 50, 400),
                                   (3, 200, 64), (7, 5, 3)])
def test_oracle_long_arms_ragged_shapes(sd, H, W, D):
    """L in {15, 20, 28, 32} x 1, 2 and 3 iterations, both views, against the CPU oracle: widths below and not a multiple
    of the pixel group (2), heights below the arm limit, one to four 128-disparity chunks, D not a multiple of 4.  (The
    oracle's n iterations are n single iterations fed their own output - it is deterministic - so it runs 3 per case,
    not 6.)"""
    import oracle as o
    import synthetic
    rng = np.random.default_rng(H * 1000 + W)
    L = blocks(H, W)
    R = synthetic.make_pair(H, W, min(16, W - 2), seed=W, kind="flat")[1]
    vl = (rng.random((D, H, W), dtype=np.float32) * 3 - 2).astype(np.float32)
    vr = (rng.random((D, H, W), dtype=np.float32) * 3 - 2).astype(np.float32)
    for dist in (15, 20, 28, 32):
        if W >= 40:
            longest, share = long_arm_share(L, dist)
            assert longest == dist - 1 and share >= 0.5, (dist, longest, share)
        ol, orr = vl, vr
        for n in (1, 2, 3):
            ol, orr = o.cost_volume_aggregation(L, R, ol, orr, TAU, dist, 1)
            assert_bits(_agg(sd, vl, L, dist, n), ol, "blocks, L=%d, %d iteration(s)" % (dist, n))
            assert_bits(_agg(sd, vr, R, dist, n), orr, "flat scene, L=%d, %d iteration(s)" % (dist, n))


# ---- 2. every slot in use -------------------------------------------------------------------------------------------
def test_oracle_long_arms_every_window_slot(sd):
    """A constant image at L = 32: arms of 31 and 63 x 63 = 3969-pixel regions, every window slot in use; and a striped
    one."""
    import oracle as o
    rng = np.random.default_rng(1)
    H, W, D = 70, 75, 5
    L = np.zeros((H, W, 1), np.float32)
    R = np.zeros((H, W, 1), np.float32)
    R[:, ::7] = 1.0
    arms, cnt = o.cross_arms(L, TAU, 32)
    assert int(arms.max()) == 31 and int(cnt.max()) == 63 * 63
    vl = rng.standard_normal((D, H, W)).astype(np.float32)
    vr = rng.standard_normal((D, H, W)).astype(np.float32)
    ol, orr = o.cost_volume_aggregation(L, R, vl, vr, TAU, 32, 2)
    assert_bits(_agg(sd, vl, L, 32, 2), ol, "constant image, distance 32")
    assert_bits(_agg(sd, vr, R, 32, 2), orr, "striped image, distance 32")


# ---- 3. special values ----------------------------------------------------------------------------------------------
def test_long_arms_special_values(sd):
    """inf / nan / signed zeros at L = 28, the plane-major reference-order kernel as the witness (the comparison of
    test_cbca_pixel_major_special_values)."""
    import _hipabi as hip
    rng = np.random.default_rng(3)
    H, W, D = 40, 66, 9
    img = np.floor(rng.random((H, W), dtype=np.float32) * 3) * np.float32(0.01)
    img[:, 20:] = blocks(H, W)[:, 20:, 0]                 # long arms right of column 20, ragged ones left of it
    assert long_arm_share(img[:, :, None], 28)[0] == 27
    sup = sd.cross_arms(dev(img), TAU, 28)
    v = rng.standard_normal((D, H, W)).astype(np.float32)
    v[0, 5, 7] = np.inf
    v[1, 9, 30] = -np.inf
    v[2, 20, 40] = np.nan
    v[3] = -0.0
    v[4, ::2] = 0.0
    vd = dev(v)
    ref, _ = sd.cbca(vd.clone(), torch.empty_like(vd), sup, 2, 28, hip.MCCNN_CBCA_REFERENCE_ORDER)
    hv = sd.dhw_to_hwd(vd)
    got, _ = sd.cbca_hwd(hv, torch.empty_like(hv), sup, D, 2, 28)
    a, b = sd.hwd_to_dhw(got, D).cpu().numpy(), ref.cpu().numpy()
    assert np.isnan(b).any() and np.isinf(b).any()
    assert np.array_equal(a.view(np.uint32) | (np.isnan(a) * 0xFFFFFFFF).astype(np.uint32),
                          b.view(np.uint32) | (np.isnan(b) * 0xFFFFFFFF).astype(np.uint32))


# ---- 4. real widths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", [(750, 40, 256), (1242, 32, 192), (1500, 24, 400), (2880, 16, 64)])
def test_long_arms_real_widths_equal_plane_major(sd, W, H, D):
    """One iteration at L = 28 through the pair launch - the block pattern as the left image, a `flat` scene as the right
    one - bit-identical to the plane-major reference-order kernel."""
    import _hipabi as hip
    import synthetic
    dist = 28
    Lb = blocks(H, W)
    fl, fr = synthetic.make_pair(H, W, min(D, W - 2), seed=1, kind="flat")[:2]
    longest, share = long_arm_share(Lb, dist)
    assert longest == dist - 1 and share >= 0.5, (longest, share)
    for view in (fl, fr):
        longest, share = long_arm_share(view, dist)
        assert longest == 27 and share >= 0.05, (longest, share)
    sl, sr = sd.cross_arms_pair(dev(Lb[:, :, 0]), dev(fr[:, :, 0]), TAU, dist)
    g = torch.Generator(device="cuda").manual_seed(W)
    a = -torch.rand((D, H, W), device="cuda", generator=g) * 50
    b = -torch.rand((D, H, W), device="cuda", generator=g) * 50
    ra, _ = sd.cbca(a.clone(), torch.empty_like(a), sl, 1, dist, hip.MCCNN_CBCA_REFERENCE_ORDER)
    rb, _ = sd.cbca(b.clone(), torch.empty_like(b), sr, 1, dist, hip.MCCNN_CBCA_REFERENCE_ORDER)
    ha, hb = sd.dhw_to_hwd(a), sd.dhw_to_hwd(b)
    (ga, _), (gb, _) = sd.cbca_hwd_pair(ha, torch.full_like(ha, float("nan")), sl, hb, torch.full_like(hb, float("nan")), sr,
                                        D, 1, dist)
    assert_bits(sd.hwd_to_dhw(ga, D).cpu().numpy(), ra.cpu().numpy(), "left volume (blocks)")
    assert_bits(sd.hwd_to_dhw(gb, D).cpu().numpy(), rb.cpu().numpy(), "right volume (flat scene)")


# ---- 5. L <= 14 through the new entry point -------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [1, 6, 14])
def test_long_entry_point_equals_hwd_up_to_14(sd, dist):
    import synthetic
    H, W, D = 45, 101, 130
    img = synthetic.make_pair(H, W, 16, seed=7, kind="flat")[0]
    sup = sd.cross_arms(dev(img[:, :, 0]), TAU, dist)
    g = torch.Generator(device="cuda").manual_seed(dist)
    v = torch.rand((D, H, W), device="cuda", generator=g) - 0.5
    hv = sd.dhw_to_hwd(v)
    want, _ = sd.cbca_hwd(hv, torch.empty_like(hv), sup, D, 2, dist)
    assert_bits(_long(sd, v, sup, dist, 2).cpu().numpy(), sd.hwd_to_dhw(want, D).cpu().numpy(), "L=%d" % dist)


# ---- 6. ABI errors --------------------------------------------------------------------------------------------------
def test_long_arms_abi_error_behaviour(sd):
    import _hipabi as hip
    lib = hip.load()
    H, W, D = 8, 16, 4
    sup = sd.cross_arms(torch.zeros((H, W), device="cuda"), TAU, 32)
    a = torch.zeros((H, W, 4), device="cuda")
    b, c, d = torch.zeros_like(a), torch.zeros_like(a), torch.zeros_like(a)
    st = hip.stream()
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), hip.ptr(sup), D, H, W, 33, st) == hip.MCCNN_E_UNSUPPORTED
    assert b"L=33" in lib.mccnn_last_error_string()
    assert lib.mccnn_cbca_iter_hwd_long_pair(hip.ptr(a), hip.ptr(b), hip.ptr(sup), hip.ptr(c), hip.ptr(d), hip.ptr(sup), D,
                                             H, W, 33, st) == hip.MCCNN_E_UNSUPPORTED
    assert b"L=33" in lib.mccnn_last_error_string()
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(a), hip.ptr(sup), D, H, W, 32, st) == hip.MCCNN_E_INVALID  # aliasing
    assert lib.mccnn_cbca_iter_hwd_long_pair(hip.ptr(a), hip.ptr(b), hip.ptr(sup), hip.ptr(a), hip.ptr(b), hip.ptr(sup), D,
                                             H, W, 32, st) == hip.MCCNN_E_INVALID                               # aliasing
    assert lib.mccnn_cbca_iter_hwd_long(None, hip.ptr(b), hip.ptr(sup), D, H, W, 32, st) == hip.MCCNN_E_INVALID
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), None, D, H, W, 32, st) == hip.MCCNN_E_INVALID
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), hip.ptr(sup), D, H + 1, W, 32, st) == hip.MCCNN_E_INVALID  # other image
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), hip.ptr(sup), D, H, W, 20, st) == hip.MCCNN_E_INVALID  # built with 32
    plane0 = sup.clone()                                   # not a buffer mccnn_cross_arms wrote
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), hip.ptr(plane0), D, H, W, 32, st) == hip.MCCNN_E_INVALID
    assert lib.mccnn_cbca_iter_hwd_long(hip.ptr(a), hip.ptr(b), hip.ptr(sup), D, H, W, 32, st) == 0
    assert lib.mccnn_cbca_iter_hwd_long_pair(hip.ptr(a), hip.ptr(b), hip.ptr(sup), hip.ptr(c), hip.ptr(d), hip.ptr(sup), D,
                                             H, W, 32, st) == 0
    torch.cuda.synchronize()


# ---- 7. whole pair --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(net_layers):
    import _hipabi as hip
    hip.require_device()
    from model import NET
    return NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)


def test_whole_pair_at_distance_28_against_the_oracle_and_the_plane_major_twin(sd, net):
    import oracle as o
    import synthetic
    H, W, D, dist = 96, 160, 32, 28
    hp = dict(cbca_distance=dist)
    L, R = synthetic.make_pair(H, W, D, seed=5, kind="flat")[:2]
    for view in (L, R):
        longest, share = long_arm_share(view, dist)
        assert longest == dist - 1 and share >= 0.10, (longest, share)
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    fl, fr = (t.cpu().numpy() for t in net.features_pair_hwc_split(l, r))
    assert not net.split_saturated(True)
    want = o.match_from_features(L, R, fl, fr, D, args=hp)
    short = o.match_from_features(L, R, fl, fr, D, args=dict(cbca_distance=14))
    assert float((want != short).mean()) > 0.5, "the L = 28 map must not be the L = 14 map"

    m = sd.StereoMatcher(net, hp=hp)
    assert m.pixel_major() and m.route(H, W, D) == "hwd_long"
    got = m.match(l, r, D)
    assert m.workspace(H, W, D)["progs"] is None
    assert_bits(got.cpu().numpy(), want, "match() at cbca_distance 28 against the oracle")
    twin = sd.StereoMatcher(net, hp=hp, layout="plane_major")
    assert not twin.pixel_major() and twin.route(H, W, D) == "plane_major"
    assert_bits(twin.match(l, r, D).cpu().numpy(), got.cpu().numpy(), "plane-major twin")
    assert_bits(m.match_graph(l, r, D).clone().cpu().numpy(), want, "match_graph()")
    assert_bits(m.match_graph(l, r, D).clone().cpu().numpy(), want, "match_graph() replay")
    # the stated footprint is what the workspace holds: no program buffers
    assert sd.workspace_bytes(H, W, D, True, m.workspace_cbca_kernel(H, W, D)) == sd.workspace_bytes(H, W, D, True, "hwd")


def test_whole_pair_at_distance_28_full_size_equals_the_plane_major_twin(sd, net):
    import synthetic
    H, W, D = 500, 750, 256
    hp = dict(cbca_distance=28)
    L, R = synthetic.make_pair(H, W, D, seed=100)[:2]
    l, r = dev(L[:, :, 0]), dev(R[:, :, 0])
    m = sd.StereoMatcher(net, hp=hp)
    assert m.pixel_major()
    got = m.match(l, r, D).cpu().numpy()
    assert m.workspace(H, W, D)["progs"] is None
    del m
    twin = sd.StereoMatcher(net, hp=hp, layout="plane_major")
    assert_bits(twin.match(l, r, D).cpu().numpy(), got, "750x500x256 at cbca_distance 28: plane-major twin")


# ---- 8. CLI ---------------------------------------------------------------------------------------------------------
def _write_pair(dirname, H, W, ndisp, seed):
    from PIL import Image
    import synthetic
    os.makedirs(dirname)
    L, R, _, _, _ = synthetic.make_pair(H, W, ndisp, seed=seed, kind="flat")
    for name, img in (("im0.png", L), ("im1.png", R)):
        g = img[:, :, 0]
        g8 = np.clip((g - g.min()) / (g.max() - g.min()) * 255.0, 0, 255).astype(np.uint8)
        Image.fromarray(g8, mode="L").save(os.path.join(dirname, name))
    with open(os.path.join(dirname, "calib.txt"), "w") as f:
        f.write("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
                "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (W, H, ndisp, ndisp))


def test_match_cli_at_distance_28_with_and_without_pipeline(tmp_path, net_layers):
    """match.py --cbca_distance 28 on a two-pair list: the same three files with and without --pipeline, and the map
    within test_cli_gpu.py's bound of the CPU checker's (99.9 % of the pixels within 1e-3 px)."""
    import oracle as o
    import util
    data = tmp_path / "data"
    H, W, D = 64, 96, 16
    rels = ["trainingH/pairA", "trainingH/pairB"]
    for i, rel in enumerate(rels):
        _write_pair(str(data / rel), H, W, D, seed=30 + i)
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in rels))
    outs = {}
    for name, extra in (("plain", []), ("pipe", ["--pipeline"])):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0",
               "--list_file", str(lst), "--resume", os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz"),
               "--data_dir", str(data), "--save_dir", str(out), "-t", "t1", "-s", "0", "-e", "1",
               "--cbca_distance", "28"] + extra
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        outs[name] = out
    for rel in rels:
        files = {}
        for name, out in outs.items():
            res = out / "submit_t1" / rel
            img = out / "submit_t1_imgs" / rel
            assert (res / "disp0MCCNN.pfm").is_file() and (res / "timeMCCNN.txt").is_file()
            assert (img / "disp0MCCNN.pgm").is_file()
            assert float((res / "timeMCCNN.txt").read_text().strip()) > 0.0
            files[name] = ((res / "disp0MCCNN.pfm").read_bytes(), (img / "disp0MCCNN.pgm").read_bytes())
        assert files["plain"] == files["pipe"], "%s: --pipeline wrote other files" % rel
        disp = util.readPfm(str(outs["plain"] / "submit_t1" / rel / "disp0MCCNN.pfm"))
        disp = disp[0] if isinstance(disp, tuple) else disp
        disp = np.asarray(disp, np.float32).reshape(H, W)
        imgs = []
        for name in ("im0.png", "im1.png"):
            g = util.read_gray(str(data / rel / name)).astype(np.float32)
            imgs.append(np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2))
        assert long_arm_share(imgs[0], 28)[0] == 27
        want = o.match_pair(imgs[0], imgs[1], D, net_layers, args=dict(cbca_distance=28))
        close = np.isclose(disp, want, atol=1e-3, equal_nan=True).mean()
        assert close >= 0.999, "%s: only %.4f of pixels within 1e-3 px of the CPU checker" % (rel, close)
