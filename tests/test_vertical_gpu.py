"""GPU: the cost volume's vertical search through every layer - mccnn_cost_volume_vertical_hwd on the edges of its
kernel, the StereoMatcher extra vertical_range stage by stage, process_functional.VERTICAL_RANGE and match.py
--vertical_range.  Everything is compared by uint32 pattern (helpers.assert_bits) with tests/vertical_reference.py,
which tests/test_vertical_cpu.py ties to the pinned oracle at range 0."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits, first_differing_stage, module_setting, stagewise
import vertical_reference as vr

pytestmark = pytest.mark.gpu

RANGES = (0, 1, 2, 4)
SENTINEL = 7.25          # what the volumes hold before a call: the pad lanes d >= D must keep it


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


def _features(H, W, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((H, W, 64)).astype(np.float32), rng.standard_normal((H, W, 64)).astype(np.float32))


def _vertical(sd, fl, fr, D, r):
    """The entry point on sentinel-filled volumes -> (left, right) [H,W,Dp] on the host."""
    H, W, _ = fl.shape
    out = tuple(torch.full((H, W, sd.hwd_pitch(D)), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2))
    got = sd.cost_volume_vertical_hwd(torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda(), D, r, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _plain(sd, fl, fr, D):
    H, W, _ = fl.shape
    out = tuple(torch.full((H, W, sd.hwd_pitch(D)), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2))
    sd.cost_volume_hwd(torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda(), D, out=out)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _against_restatement(sd, fl, fr, D, r, what):
    got = _vertical(sd, fl, fr, D, r)
    want = vr.compute_cost_volume_vertical(fl, fr, D, r)
    for side in (0, 1):
        assert_bits(vr.hwd_to_dhw(got[side], D), want[side], "%s, range %d, %s volume" % (what, r, ("left", "right")[side]))
    return got, want


# (1,8,2): one row, every k != 0 skipped; (2,10,3): fewer rows than 2r + 1; (3,66,64): the 63-pixel tile seam and the
# ghost lane; (5,130,65): padded Dp; (9,200,198): D = W - 2; (4,300,257): several 64-disparity tiles, the ring's reuse;
# (6,1030,1024): all four SGM disparity groups' worth of lanes
@pytest.mark.parametrize("H,W,D", [(1, 8, 2), (2, 10, 3), (3, 66, 64), (5, 130, 65), (9, 200, 198), (4, 300, 257),
                                   (6, 1030, 1024)])
def test_entry_point_equals_the_restatement(sd, H, W, D):
    fl, fr = _features(H, W, 100 + H)
    plain = _plain(sd, fl, fr, D)
    for r in RANGES:
        got, _ = _against_restatement(sd, fl, fr, D, r, "%dx%dx%d" % (H, W, D))
        for side in (0, 1):
            assert_bits(got[side][:, :, D:], plain[side][:, :, D:], "pad lanes, range %d, side %d" % (r, side))
            assert (got[side][:, :, D:] == SENTINEL).all()


@pytest.mark.parametrize("H,W,D", [(5, 130, 65), (4, 300, 257)])
def test_range_0_equals_the_plain_entry_point(sd, H, W, D):
    fl, fr = _features(H, W, 7)
    got, plain = _vertical(sd, fl, fr, D, 0), _plain(sd, fl, fr, D)
    assert_bits(got[0], plain[0], "left volume, pad lanes included")
    assert_bits(got[1], plain[1], "right volume, pad lanes included")


def test_range_matters_and_the_right_volume_is_no_copy_of_the_left(sd):
    H, W, D = 5, 70, 16
    fl, fr = _features(H, W, 11)
    l0, r0 = (vr.hwd_to_dhw(v, D) for v in _vertical(sd, fl, fr, D, 0))
    l2, r2 = (vr.hwd_to_dhw(v, D) for v in _vertical(sd, fl, fr, D, 2))
    assert (l2 <= l0).all() and (l2 < l0).any()                 # costs: the negated maxima can only fall
    d = 3
    assert np.array_equal(r0[d, :, :W - d], l0[d, :, d:])
    assert not np.array_equal(r2[d, :, :W - d], l2[d, :, d:])


def test_special_values(sd):
    """NaN exactly where the definition puts it (a NaN candidate makes the score NaN, in either view, over all rows
    that search the pixel), the signs of zeros as defined, +inf as the largest score."""
    H, W, D, r = 5, 70, 16, 2
    nan, inf = np.float32("nan"), np.float32("inf")

    fl, fr = _features(H, W, 21)
    fl[2, 30, :] = nan
    _, want = _against_restatement(sd, fl, fr, D, r, "NaN pixel in the left image")
    assert np.isnan(want[0][:, 2, 30]).all() and not np.isnan(want[0][:, 0, D:]).any()
    assert np.isnan(want[1][0, 0:5, 30]).all()                  # right pixels of rows 2 -+ 2 see it at d = 0

    fl, fr = _features(H, W, 22)
    fr[1, 20, :] = nan
    _, want = _against_restatement(sd, fl, fr, D, r, "NaN pixel in the right image")
    assert np.isnan(want[1][:, 1, 20]).all() and np.isnan(want[0][0, 0:4, 20]).all()
    assert not np.isnan(want[0][:, 4, D:]).any()

    fl, fr = np.zeros((H, W, 64), np.float32), np.zeros((H, W, 64), np.float32)
    fl[:, ::3, ::2] = -0.0
    fr[::2, :, 1::2] = -0.0
    _against_restatement(sd, fl, fr, D, r, "all-zero images with -0.0 among the features")

    fl, fr = _features(H, W, 23)
    fl[3, 40, 5] = inf
    _, want = _against_restatement(sd, fl, fr, D, r, "one +inf feature")
    assert np.isinf(want[0][:, 3, 40]).all()


# ---- the matcher -----------------------------------------------------------------------------------------------------
def _off_pair(H, W, D, seed):
    """A synthetic pair whose right image sits two rows low: (L, R) standardised [H,W,1], and their bytes."""
    import synthetic
    l8, r8, _ = synthetic.make_scene_u8(H, W, D, seed)
    r8 = vr.shift_rows(r8, 2)
    return synthetic.standardize(l8), synthetic.standardize(r8), l8, r8


@pytest.mark.parametrize("H,W,D", [(40, 48, 16), (24, 130, 64)])
def test_matcher_stage_by_stage(sd, net, H, W, D):
    import oracle as o
    L, R, l8, r8 = _off_pair(H, W, D, seed=5)
    l, r = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = sd.StereoMatcher(net, extras=dict(vertical_range=2))
    keep = {}
    out = m.match(l, r, D, keep=keep).cpu().numpy()
    assert m.features == "split_f16" and not m.features_saturated()
    # the kept cost volumes: the restatement on the GPU's own features
    fl, fr = (t.cpu().numpy() for t in net.features_pair_hwc_split(l[:, :, 0].contiguous(), r[:, :, 0].contiguous()))
    want = vr.compute_cost_volume_vertical(fl, fr, D, 2)
    assert_bits(keep["cv"][0].cpu().numpy(), want[0], "kept left cost volume")
    assert_bits(keep["cv"][1].cpu().numpy(), want[1], "kept right cost volume")
    plain = o.compute_cost_volume(fl, fr, D)
    assert not np.array_equal(plain[0], want[0])
    # everything behind them: the oracle chain fed the GPU's volumes
    d = stagewise(keep, L, R, D, o)
    assert first_differing_stage(d) is None, d
    assert_bits(out, keep["bilateral"].cpu().numpy(), "the returned map is the last stage")
    # every entry gives these bits
    assert_bits(m.match(l, r, D).cpu().numpy(), out, "match without keep")
    g = sd.StereoMatcher(net, extras=dict(vertical_range=2))
    for what in ("capture", "replay", "second replay"):
        assert_bits(g.match_graph(l, r, D).cpu().numpy(), out, "match_graph (%s)" % what)
    assert len(g._graphs) == 1
    assert_bits(m.match_u8(torch.from_numpy(l8).cuda(), torch.from_numpy(r8).cuda(), D).cpu().numpy(), out, "match_u8")
    # range 0 is the matcher without the extra; the range changes the map of this pair
    without = sd.StereoMatcher(net).match(l, r, D).cpu().numpy()
    assert_bits(sd.StereoMatcher(net, extras=dict(vertical_range=0)).match(l, r, D).cpu().numpy(), without, "range 0")
    assert not np.array_equal(without, out)
    both = sd.StereoMatcher(net, extras=dict(vertical_range=2), views="both").match(l, r, D).cpu().numpy()
    assert both.shape == (2, H, W)
    assert_bits(both[0], out, "views='both': the left map")


def test_process_functional_switch(sd):
    import process_functional as pf
    H, W, D = 6, 40, 12
    fl, fr = _features(H, W, 31)
    with module_setting(pf, "VERTICAL_RANGE", 2):
        got = pf.compute_cost_volume(fl, fr, D)
        with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
            with pytest.raises(ValueError, match="'exact' only"):
                pf.compute_cost_volume(fl, fr, D)
    want = vr.compute_cost_volume_vertical(fl, fr, D, 2)
    assert got[0].shape == (D, H, W) and isinstance(got[0], np.ndarray)
    assert_bits(got[0], want[0], "left")
    assert_bits(got[1], want[1], "right")
    assert pf.VERTICAL_RANGE == 0
    plain = vr.compute_cost_volume_vertical(fl, fr, D, 0)
    assert_bits(pf.compute_cost_volume(fl, fr, D)[0], plain[0], "switch off")


# ---- match.py --------------------------------------------------------------------------------------------------------
CLI_H, CLI_W, CLI_D = 32, 64, 16
RELS = ["trainingH/pairA", "trainingH/pairB"]


def _tree(tmp_path):
    from PIL import Image
    data, lst = tmp_path / "data", tmp_path / "list.txt"
    for i, rel in enumerate(RELS):
        _, _, l8, r8 = _off_pair(CLI_H, CLI_W, CLI_D, seed=60 + i)
        os.makedirs(str(data / rel))
        for name, img in (("im0.png", l8), ("im1.png", r8)):
            Image.fromarray(np.ascontiguousarray(img), mode="L").save(str(data / rel / name))
        (data / rel / "calib.txt").write_text(
            "cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\nwidth=%d\nheight=%d\nndisp=%d\n"
            "isint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (CLI_W, CLI_H, CLI_D, CLI_D))
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in RELS))
    return data, lst


def _cli(tmp_path, data, lst, tag, extra):
    cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0", "--list_file", str(lst),
           "--data_dir", str(data), "--save_dir", str(tmp_path / "out"), "-t", tag, "-s", "0", "-e", "1", "--resume",
           os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")] + extra
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)


def _files(tmp_path, tag):
    return [(tmp_path / "out" / ("submit_%s" % tag) / rel / "disp0MCCNN.pfm").read_bytes() for rel in RELS]


def test_match_cli(tmp_path):
    data, lst = _tree(tmp_path)
    written = {}
    for tag, extra in (("plain", []), ("v", ["--vertical_range", "2"]),
                       ("vf", ["--vertical_range", "2", "--pairs_in_flight", "2"]),
                       ("vp", ["--vertical_range", "2", "--pipeline"])):
        r = _cli(tmp_path, data, lst, tag, extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        written[tag] = _files(tmp_path, tag)
    for k in range(len(RELS)):
        assert written["v"][k] == written["vf"][k], "%s: --pairs_in_flight 2 wrote another map" % RELS[k]
        assert written["v"][k] == written["vp"][k], "%s: --pipeline wrote another map" % RELS[k]
        assert written["v"][k] != written["plain"][k], "%s: --vertical_range 2 changed nothing" % RELS[k]
    for flags, reason in ((["--fast"], "--fast"), (["--separable_cbca"], "--separable_cbca"),
                          (["--arch", "accurate"], "--arch accurate")):
        r = _cli(tmp_path, data, lst, "refused", ["--vertical_range", "2"] + flags)
        assert r.returncode != 0
        assert "--vertical_range is not available with %s" % reason in r.stdout.decode()
