"""GPU: a pair's row offset through every layer - mccnn_cost_volume_offset_hwd, mccnn_vertical_profile and
mccnn_vertical_offset_select on the edges of their kernels, the StereoMatcher extras vertical_offset*, the module switch
of process_functional and match.py --vertical_offset.  Everything is compared by uint32 pattern (helpers.assert_bits) or
as integers with tests/vertical_offset_reference.py, which tests/test_vertical_offset_cpu.py ties to
tests/vertical_reference.py and the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits, first_differing_stage, module_setting, stagewise
import vertical_offset_reference as vo
import vertical_reference as vr

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345          # a NaN pattern: what every output holds before a call
RAGGED = (7, 130, 70)        # three 63-pixel tiles, the last one ragged; two disparity tiles; D % 4 != 0
MINIMAL = [(3, 6, 2), (1, 4, 2)]
THREE_TILES = (20, 200, 129)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


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


_FEATURES = {}


def _features(H, W, seed=None):
    key = (H, W, seed)
    if key not in _FEATURES:
        rng = np.random.RandomState(1000 + 7 * H + W if seed is None else seed)
        _FEATURES[key] = (rng.standard_normal((H, W, 64)).astype(np.float32),
                          rng.standard_normal((H, W, 64)).astype(np.float32))
    return _FEATURES[key]


def _poisoned(shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _k0(value):
    return torch.tensor([value], dtype=torch.int32, device="cuda")


def _offset_volumes(sd, fl, fr, D, k0, r):
    """The entry point on poisoned volumes -> (left, right) [H,W,Dp] on the host; k0: an int, or None for a null pointer."""
    H, W, _ = fl.shape
    out = (_poisoned((H, W, sd.hwd_pitch(D))), _poisoned((H, W, sd.hwd_pitch(D))))
    got = sd.cost_volume_offset_hwd(torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda(), D,
                                    None if k0 is None else _k0(k0), r, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _check_offset(sd, fl, fr, D, k0, r, what):
    got = _offset_volumes(sd, fl, fr, D, k0, r)
    want = vo.compute_cost_volume_offset(fl, fr, D, k0, r)
    for side in (0, 1):
        label = "%s, offset %d, range %d, %s volume" % (what, k0, r, ("left", "right")[side])
        assert_bits(vr.hwd_to_dhw(got[side], D), want[side], label)
        assert (got[side][:, :, D:].view(np.uint32) == POISON).all(), label + ": a pad entry was written"
    return got, want


# ---- the offset volume -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0", [-8, -3, 0, 2, 8])
def test_offset_volume_ragged_shape(sd, k0):
    """At +-8 every row of the 7 is clamped to the nearest image row."""
    H, W, D = RAGGED
    fl, fr = _features(H, W)
    for r in (0, 1, 4):
        _check_offset(sd, fl, fr, D, k0, r, "%dx%dx%d" % RAGGED)


@pytest.mark.parametrize("H,W,D", MINIMAL)
def test_offset_volume_minimal_shapes(sd, H, W, D):
    fl, fr = _features(H, W)
    for k0 in (-8, -1, 0, 1, 2):
        for r in (0, 1, 4):
            _check_offset(sd, fl, fr, D, k0, r, "%dx%dx%d" % (H, W, D))


def test_offset_volume_three_disparity_tiles(sd):
    H, W, D = THREE_TILES
    fl, fr = _features(H, W)
    for r in (0, 1):
        _check_offset(sd, fl, fr, D, 3, r, "%dx%dx%d" % THREE_TILES)


def test_offset_volume_special_values(sd):
    H, W, D, k0, r = 6, 70, 16, 2, 1
    nan = np.float32("nan")
    fl, fr = (a.copy() for a in _features(H, W, seed=21))
    fl[2, 30, :] = nan
    _, want = _check_offset(sd, fl, fr, D, k0, r, "NaN pixel in the left image")
    assert np.isnan(want[0][:, 2, 30]).all() and not np.isnan(want[0][:, 0, D:]).any()
    assert np.isnan(want[1][0, 3:6, 30]).all()                  # right rows 2 + (k0 -+ r) see it at d = 0
    fl, fr = (a.copy() for a in _features(H, W, seed=22))
    fr[4, 20, :] = nan
    _, want = _check_offset(sd, fl, fr, D, k0, r, "NaN pixel in the right image")
    assert np.isnan(want[1][:, 4, 20]).all() and np.isnan(want[0][0, 1:4, 20]).all()
    fl, fr = np.zeros((H, W, 64), np.float32), np.zeros((H, W, 64), np.float32)
    fl[:, ::3, ::2] = -0.0
    fr[::2, :, 1::2] = -0.0
    for kk in (-8, 0, 2):
        _check_offset(sd, fl, fr, D, kk, r, "all-zero images with -0.0 among the features")


def test_offset_volume_memory_contract(sd):
    """Poisoned pads stay, bases that are 4-byte but not 16-byte aligned, the red zones around both volumes intact."""
    H, W, D = RAGGED
    dp, zone = sd.hwd_pitch(D), 16384
    fl, fr = _features(H, W)
    n, nf = H * W * dp, H * W * 64
    arena = torch.full((4 * zone + 2 * n + 2 * nf + 16,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    at = [zone + 1]                                              # float offsets: 4, 12, 4, 8 bytes past a 16-byte boundary
    at.append(at[0] + n + zone + 2)
    at.append(at[1] + n + zone + 2)
    at.append(at[2] + nf + 5)
    assert [(arena.data_ptr() + 4 * a) % 16 for a in at] == [4, 12, 4, 8]
    left, right = arena[at[0]:at[0] + n].view(H, W, dp), arena[at[1]:at[1] + n].view(H, W, dp)
    dfl, dfr = arena[at[2]:at[2] + nf].view(H, W, 64), arena[at[3]:at[3] + nf].view(H, W, 64)
    dfl.copy_(torch.from_numpy(fl))
    dfr.copy_(torch.from_numpy(fr))
    before = arena.view(torch.int32).cpu().numpy().copy()
    for k0, r in ((2, 1), (-8, 0)):
        left.view(torch.int32).fill_(POISON)
        right.view(torch.int32).fill_(POISON)
        sd.cost_volume_offset_hwd(dfl, dfr, D, _k0(k0), r, out=(left, right))
        want = vo.compute_cost_volume_offset(fl, fr, D, k0, r)
        after = arena.view(torch.int32).cpu().numpy()
        written = np.zeros(after.shape, bool)
        for a, w in zip(at[:2], want):
            vol = after[a:a + n].reshape(H, W, dp)
            assert_bits(vr.hwd_to_dhw(vol.view(np.float32), D), w, "offset %d, range %d at an odd base" % (k0, r))
            assert (vol[:, :, D:] == POISON).all(), "a pad entry was written"
            written[a:a + n] = True
        assert np.array_equal(after[~written], before[~written]), "a byte outside the volumes changed"


def test_offset_pointer(sd):
    H, W, D = RAGGED
    fl, fr = _features(H, W)
    for stored, acts_as in ((INT32_MAX, 8), (INT32_MIN, -8), (9, 8), (-1000, -8)):
        got = _offset_volumes(sd, fl, fr, D, stored, 1)
        want = _offset_volumes(sd, fl, fr, D, acts_as, 1)
        assert_bits(got[0], want[0], "a stored %d behaves as %d (left)" % (stored, acts_as))
        assert_bits(got[1], want[1], "a stored %d behaves as %d (right)" % (stored, acts_as))
    for r in (0, 2):
        out = (_poisoned((H, W, sd.hwd_pitch(D))), _poisoned((H, W, sd.hwd_pitch(D))))
        sd.cost_volume_vertical_hwd(torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda(), D, r, out=out)
        for k0 in (None, 0):
            got = _offset_volumes(sd, fl, fr, D, k0, r)
            for side in (0, 1):
                assert_bits(got[side], out[side].cpu().numpy(), "offset %r, range %d == the vertical search" % (k0, r))


# ---- profile and select ------------------------------------------------------------------------------------------------
PROFILES = [(0, 1), (1, 2), (4, 1), (8, 8)]


def _profile(sd, fl, fr, D, R, step):
    """-> (votes uint32, offset int, totals uint64) of the device, from buffers pre-filled with garbage."""
    H, W, _ = fl.shape
    votes = torch.full(sd.vertical_profile_shape(H, W, R, step), -1234567, dtype=torch.int32, device="cuda")
    got = sd.vertical_profile(torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda(), D, R, step, out=votes)
    assert got is votes
    offset = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    totals = torch.full((2 * R + 1,), -5, dtype=torch.int64, device="cuda")
    sd.vertical_offset_select(votes, R, out=(offset, totals))
    return votes.cpu().numpy().view(np.uint32), int(offset.cpu().numpy()[0]), totals.cpu().numpy().view(np.uint64)


def _check_profile(sd, fl, fr, D, R, step, what):
    votes, offset, totals = _profile(sd, fl, fr, D, R, step)
    want = vo.vertical_profile(fl, fr, D, R, step)
    label = "%s, max %d, step %d" % (what, R, step)
    assert votes.shape == want.shape and np.array_equal(votes, want), label + ": votes"
    want_offset, want_totals = vo.offset_select(want, R)
    assert np.array_equal(totals, want_totals), label + ": totals"
    assert offset == want_offset, label + ": offset"
    return want


@pytest.mark.parametrize("H,W,D", [RAGGED] + MINIMAL + [THREE_TILES])
def test_profile_and_select_equal_the_restatement(sd, H, W, D):
    fl, fr = _features(H, W)
    for R, step in PROFILES:
        want = _check_profile(sd, fl, fr, D, R, step, "%dx%dx%d" % (H, W, D))
        assert int(want.sum()) == vo.profile_rows(H, step) * W          # finite features: every profiled pixel votes


def test_profile_finds_a_shifted_row_and_skips_nan_pixels(sd):
    H, W, D = 12, 130, 20
    fl, _ = _features(H, W, seed=31)
    fr = np.zeros_like(fl)
    fr[:, :W - 3] = fl[:, 3:]                                    # disparity 3 ...
    fr = vr.shift_rows(fr, 2)                                    # ... two rows low
    want = _check_profile(sd, fl, fr, D, 4, 2, "shifted copy")
    assert vo.offset_select(want, 4)[0] == 2
    fl2 = fl.copy()
    fl2[3, 5:9, 0] = np.float32("nan")                           # four pixels of profiled row 3 (step 2: rows 1, 3, ...)
    fr2 = fr.copy()
    fr2[10, :, 1] = np.float32("nan")                            # a whole right row: rows 7, 9, 11 see it within +-4
    want = _check_profile(sd, fl2, fr2, D, 4, 2, "NaN pixels")
    assert [int(want[i].sum()) for i in range(6)] == [W, W - 4, W, 0, 0, 0]
    zeros = np.zeros((5, 70, 64), np.float32)
    want = _check_profile(sd, zeros, zeros, 8, 3, 1, "flat image")
    assert int(want[:, :, 3].sum()) == 5 * 70                   # a flat image votes 0
    empty = torch.zeros((2, 3, 9), dtype=torch.int32, device="cuda")
    offset, totals = sd.vertical_offset_select(empty, 4)
    assert int(offset.cpu()[0]) == 0 and not totals.cpu().numpy().any()       # no votes at all: 0


# ---- the matcher -------------------------------------------------------------------------------------------------------
PAIR = (40, 96, 24)


def _off_pair(H, W, D, seed, dy=2):
    """A synthetic pair whose right image sits dy rows low: (L, R) standardised [H,W,1], and their bytes."""
    import synthetic
    l8, r8, _ = synthetic.make_scene_u8(H, W, D, seed)
    r8 = vr.shift_rows(r8, dy)
    return synthetic.standardize(l8), synthetic.standardize(r8), l8, r8


@pytest.fixture(scope="module")
def pair(sd, net):
    """The pair on the device, its features on the host and the restated volumes at offset 2, ranges 0 and 1."""
    H, W, D = PAIR
    L, R, l8, r8 = _off_pair(H, W, D, seed=5)
    l, r = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    fl, fr = (t.cpu().numpy() for t in net.features_pair_hwc_split(l[:, :, 0].contiguous(), r[:, :, 0].contiguous()))
    want = {rng: vo.compute_cost_volume_offset(fl, fr, D, 2, rng) for rng in (0, 1)}
    return dict(L=L, R=R, l=l, r=r, l8=l8, r8=r8, fl=fl, fr=fr, want=want)


def _stages(sd, net, pair, extras, want, what, **kw):
    """match(keep=) of a matcher with `extras`: kept volumes == `want`, every later stage == the CPU chain."""
    import oracle as o
    H, W, D = PAIR
    m = sd.StereoMatcher(net, extras=extras, **kw)
    keep = {}
    out = m.match(pair["l"], pair["r"], D, keep=keep)
    out = out.cpu().numpy()
    assert m.features == "split_f16" and not m.features_saturated()
    assert_bits(keep["cv"][0].cpu().numpy(), want[0], what + ": kept left cost volume")
    assert_bits(keep["cv"][1].cpu().numpy(), want[1], what + ": kept right cost volume")
    d = stagewise(keep, pair["L"], pair["R"], D, o)
    assert first_differing_stage(d) is None, (what, d)
    left = out[0] if kw.get("views") == "both" else out
    assert_bits(left, keep["bilateral"].cpu().numpy(), what + ": the returned map is the last stage")
    return m, out


def test_matcher_integer_offset(sd, net, pair):
    H, W, D = PAIR
    m, out = _stages(sd, net, pair, dict(vertical_offset=2), pair["want"][0], "vertical_offset=2")
    assert_bits(m.match(pair["l"], pair["r"], D).cpu().numpy(), out, "match without keep")
    g = sd.StereoMatcher(net, extras=dict(vertical_offset=2))
    for what in ("capture", "replay", "second replay"):
        assert_bits(g.match_graph(pair["l"], pair["r"], D).cpu().numpy(), out, "match_graph (%s)" % what)
    assert len(g._graphs) == 1
    assert_bits(m.match_u8(torch.from_numpy(pair["l8"]).cuda(), torch.from_numpy(pair["r8"]).cuda(), D).cpu().numpy(), out,
                "match_u8")
    assert m.vertical_report(H, W, D) == dict(offset=2, totals=[0] * 9, share=0.0)
    without = sd.StereoMatcher(net).match(pair["l"], pair["r"], D).cpu().numpy()
    assert not np.array_equal(without, out)


def test_matcher_auto(sd, net, pair):
    H, W, D = PAIR
    fixed = sd.StereoMatcher(net, extras=dict(vertical_offset=2)).match(pair["l"], pair["r"], D).cpu().numpy()
    extras = dict(vertical_offset="auto", vertical_offset_max=4, vertical_offset_rows=4)
    m, out = _stages(sd, net, pair, extras, pair["want"][0], "vertical_offset='auto'")
    assert_bits(out, fixed, "'auto' == vertical_offset=2")
    votes = vo.vertical_profile(pair["fl"], pair["fr"], D, 4, 4)
    offset, totals = vo.offset_select(votes, 4)
    assert offset == 2
    want_report = dict(offset=2, totals=[int(t) for t in totals], share=vo.share(totals, 2, 4))
    assert m.vertical_report(H, W, D) == want_report
    assert_bits(m.match(pair["l"], pair["r"], D).cpu().numpy(), out, "match without keep")
    g = sd.StereoMatcher(net, extras=extras)
    for what in ("capture", "replay", "second replay"):
        assert_bits(g.match_graph(pair["l"], pair["r"], D).cpu().numpy(), out, "match_graph (%s)" % what)
        assert g.vertical_report(H, W, D) == want_report, what
    assert len(g._graphs) == 1


def test_matcher_both_views_and_range(sd, net, pair):
    H, W, D = PAIR
    fixed = sd.StereoMatcher(net, extras=dict(vertical_offset=2)).match(pair["l"], pair["r"], D).cpu().numpy()
    both = sd.StereoMatcher(net, extras=dict(vertical_offset="auto", vertical_offset_rows=4), views="both")
    both = both.match(pair["l"], pair["r"], D).cpu().numpy()
    assert both.shape == (2, H, W)
    assert_bits(both[0], fixed, "views='both': the left map")
    both2 = sd.StereoMatcher(net, extras=dict(vertical_offset=2), views="both").match(pair["l"], pair["r"], D)
    assert_bits(both, both2.cpu().numpy(), "views='both': 'auto' == vertical_offset=2")
    m, out = _stages(sd, net, pair, dict(vertical_offset=2, vertical_range=1), pair["want"][1], "offset 2, range 1")
    assert not np.array_equal(out, fixed)
    g = sd.StereoMatcher(net, extras=dict(vertical_offset="auto", vertical_offset_rows=4, vertical_range=1))
    assert_bits(g.match_graph(pair["l"], pair["r"], D).cpu().numpy(), out, "auto with range 1, captured")


def test_matcher_other_routes(sd, net, pair):
    """Long arms (cbca_distance 20: the joined long-arm aggregation), the paper's SGM, confidence planes and a sparse
    map: 'auto' gives what vertical_offset=2 gives, element by element, and not what the plain matcher gives."""
    H, W, D = PAIR
    kw = dict(hp=dict(cbca_distance=20), confidence=("msm",), semi_dense="lr")
    results = {}
    for name, extras in (("plain", {}), ("two", dict(vertical_offset=2)),
                         ("auto", dict(vertical_offset="auto", vertical_offset_rows=4))):
        m = sd.StereoMatcher(net, extras=dict(extras, sgm_independent_directions=True), **kw)
        results[name] = [t.cpu().numpy() for t in m.match(pair["l"], pair["r"], D)]
        if name == "auto":
            assert m.vertical_report(H, W, D)["offset"] == 2
    assert len(results["auto"]) == 3
    for k, what in enumerate(("map", "confidence planes", "sparse map")):
        assert_bits(results["auto"][k], results["two"][k], "long arms, paper SGM: %s" % what)
    assert not np.array_equal(results["plain"][0], results["two"][0])


def test_matcher_defaults_change_nothing(sd, net, pair):
    H, W, D = PAIR
    plain = sd.StereoMatcher(net)
    spelt = sd.StereoMatcher(net, extras=dict(vertical_offset=0, vertical_offset_max=4, vertical_offset_rows=8))
    assert_bits(spelt.match(pair["l"], pair["r"], D).cpu().numpy(), plain.match(pair["l"], pair["r"], D).cpu().numpy(),
                "the extras at their defaults")
    ws = spelt.workspace(H, W, D)
    assert not [k for k in ws if k.startswith("v_")]
    base = sd.workspace_bytes(H, W, D, True, plain.workspace_cbca_kernel(H, W, D))
    assert sd.workspace_bytes(H, W, D, True, plain.workspace_cbca_kernel(H, W, D), vertical_offset=0) == base
    rows, blocks, nk = sd.vertical_profile_shape(H, W, 4, 8)
    assert (rows, blocks, nk) == (5, 2, 9)
    on = sd.workspace_bytes(H, W, D, True, plain.workspace_cbca_kernel(H, W, D), vertical_offset="auto")
    assert on == base + 4 + 8 * nk + 4 * rows * blocks * nk
    with pytest.raises(ValueError, match="vertical_report"):
        plain.vertical_report(H, W, D)


def test_process_functional_switch(sd):
    import process_functional as pf
    H, W, D = 6, 40, 12
    fl, fr = _features(H, W, seed=31)
    with module_setting(pf, "VERTICAL_OFFSET", -2):
        got = pf.compute_cost_volume(fl, fr, D)
        with module_setting(pf, "VERTICAL_RANGE", 1):
            got1 = pf.compute_cost_volume(fl, fr, D)
        with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
            with pytest.raises(ValueError, match="'exact' only"):
                pf.compute_cost_volume(fl, fr, D)
    for g, r in ((got, 0), (got1, 1)):
        want = vo.compute_cost_volume_offset(fl, fr, D, -2, r)
        assert g[0].shape == (D, H, W) and isinstance(g[0], np.ndarray)
        assert_bits(g[0], want[0], "left, range %d" % r)
        assert_bits(g[1], want[1], "right, range %d" % r)
    assert pf.VERTICAL_OFFSET == 0
    offset, totals, votes = pf.vertical_profile(fl, fr, D, 3, 2)
    want = vo.vertical_profile(fl, fr, D, 3, 2)
    assert votes.dtype == np.uint32 and np.array_equal(votes, want)
    assert (offset, list(totals)) == (vo.offset_select(want, 3)[0], list(vo.offset_select(want, 3)[1]))


# ---- match.py ----------------------------------------------------------------------------------------------------------
CLI_H, CLI_W, CLI_D = 32, 64, 16
RELS = ["trainingH/pairA", "trainingH/pairB"]


def _tree(root, dy):
    from PIL import Image
    data, lst = root / "data", root / "list.txt"
    for i, rel in enumerate(RELS):
        _, _, l8, r8 = _off_pair(CLI_H, CLI_W, CLI_D, seed=60 + i, dy=dy)
        os.makedirs(str(data / rel))
        for name, img in (("im0.png", l8), ("im1.png", r8)):
            Image.fromarray(np.ascontiguousarray(img), mode="L").save(str(data / rel / name))
        (data / rel / "calib.txt").write_text(
            "cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\nwidth=%d\nheight=%d\nndisp=%d\n"
            "isint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n" % (CLI_W, CLI_H, CLI_D, CLI_D))
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in RELS))
    return data, lst


def _cli(root, data, lst, tag, extra):
    cmd = [sys.executable, os.path.join(ROOT, "mc-cnn-python_amd", "src", "match.py"), "-g", "0", "--list_file", str(lst),
           "--data_dir", str(data), "--save_dir", str(root / "out"), "-t", tag, "-s", "0", "-e", "1", "--resume",
           os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    out = {}
    for rel in RELS:
        d = root / "out" / ("submit_%s" % tag) / rel
        out[rel] = dict((name, (d / name).read_bytes()) for name in sorted(os.listdir(str(d))) if name != "timeMCCNN.txt")
    return out


AUTO = ["--vertical_offset", "auto", "--vertical_offset_rows", "4"]


def test_match_cli_writes_the_same_files_in_all_three_loops(tmp_path):
    data, lst = _tree(tmp_path, 2)
    written = dict((tag, _cli(tmp_path, data, lst, tag, extra)) for tag, extra in (
        ("a", AUTO), ("af", AUTO + ["--pairs_in_flight", "2"]), ("ap", AUTO + ["--pipeline"]), ("two", ["--vertical_offset", "2"])))
    for rel in RELS:
        files = written["a"][rel]
        assert sorted(files) == ["disp0MCCNN.pfm", "verticalMCCNN.json"]
        record = json.loads(files["verticalMCCNN.json"].decode())
        assert sorted(record) == ["max_offset", "offset", "row_step", "share", "totals"]
        assert (record["offset"], record["max_offset"], record["row_step"], len(record["totals"])) == (2, 4, 4, 9)
        assert sum(record["totals"]) == (CLI_H // 4) * CLI_W and record["share"] == record["totals"][6] / sum(record["totals"])
        assert written["af"][rel] == files, "%s: --pairs_in_flight 2 wrote other files" % rel
        assert written["ap"][rel] == files, "%s: --pipeline wrote other files" % rel
        # an integer offset: the same map, and no measurement
        assert written["two"][rel] == {"disp0MCCNN.pfm": files["disp0MCCNN.pfm"]}, "%s: --vertical_offset 2" % rel


def test_match_cli_a_measured_offset_of_0_changes_no_other_file(tmp_path):
    data, lst = _tree(tmp_path, 0)
    plain, measured = _cli(tmp_path, data, lst, "plain", []), _cli(tmp_path, data, lst, "a", AUTO)
    for rel in RELS:
        assert json.loads(measured[rel].pop("verticalMCCNN.json").decode())["offset"] == 0
        assert measured[rel] == plain[rel], "%s: a measured offset of 0 changed a file" % rel
