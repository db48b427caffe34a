"""GPU: a field of row offsets through every layer - mccnn_vertical_field_select and mccnn_cost_volume_field_hwd on the
edges of their kernels (volumes in tests/arena.py arenas: pads, red zones, odd bases), the StereoMatcher extra
vertical_offset="grid", the module switch of process_functional and match.py --vertical_offset grid.  Everything is
compared by uint32 pattern (helpers.assert_bits) or as integers with tests/vertical_field_reference.py, which
tests/test_vertical_field_cpu.py ties to tests/vertical_offset_reference.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arena
from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits, first_differing_stage, module_setting, stagewise
import vertical_field_reference as vf
import vertical_offset_reference as vo
import vertical_reference as vr

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31


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
        rng = np.random.RandomState(2000 + 7 * H + W if seed is None else seed)
        _FEATURES[key] = (rng.standard_normal((H, W, 64)).astype(np.float32),
                          rng.standard_normal((H, W, 64)).astype(np.float32))
    return _FEATURES[key]


# ---- the selection -----------------------------------------------------------------------------------------------------
def _select(sd, votes, H, step, R, grid):
    """The entry point on buffers pre-filled with garbage -> (field, totals uint64, offset, global totals uint64)."""
    gh, gw = grid
    out = (torch.full((gh, gw), 77, dtype=torch.int32, device="cuda"),
           torch.full((gh, gw, 2 * R + 1), -5, dtype=torch.int64, device="cuda"),
           torch.full((1,), 77, dtype=torch.int32, device="cuda"),
           torch.full((2 * R + 1,), -5, dtype=torch.int64, device="cuda"))
    dev = torch.from_numpy(votes.view(np.int32)).cuda()
    got = sd.vertical_field_select(dev, H, step, R, grid, out=out)
    assert all(g is o for g, o in zip(got, out))
    # the same votes through the shipped selection: the global outputs are exactly its
    offset, totals = sd.vertical_offset_select(dev, R)
    assert int(offset.cpu()[0]) == int(out[2].cpu()[0]) and torch.equal(totals, out[3])
    return (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint64), int(out[2].cpu()[0]),
            out[3].cpu().numpy().view(np.uint64))


def _check_select(sd, votes, H, step, R, grid, what):
    got = _select(sd, votes, H, step, R, grid)
    want = vf.field_select(votes, H, step, R, *grid)
    label = "%s, %dx%d votes, grid %dx%d" % ((what,) + votes.shape[:2] + tuple(grid))
    assert np.array_equal(got[1], want[1]), label + ": cell totals"
    assert np.array_equal(got[0], want[0]), label + ": field"
    assert got[2] == want[2] and np.array_equal(got[3], want[3]), label + ": the global winner"
    return want


# (n_rows, n_blocks): H, row_step and the grids - the largest the shape allows among them
SELECT_SHAPES = {(1, 1): (1, 1, [(1, 1)]), (3, 2): (3, 1, [(1, 1), (3, 2), (2, 1)]),
                 (24, 12): (96, 4, [(1, 1), (3, 4), (8, 8), (5, 7)])}


@pytest.mark.parametrize("shape", sorted(SELECT_SHAPES))
def test_select_equals_the_restatement(sd, shape):
    H, step, grids = SELECT_SHAPES[shape]
    for R in (0, 2, 8):
        rng = np.random.RandomState(sum(shape) + R)
        votes = rng.randint(0, 200, size=shape + (2 * R + 1,)).astype(np.uint32)
        zeros = np.zeros_like(votes)
        hot = zeros.copy()
        hot[shape[0] // 2, shape[1] - 1, 2 * R] = 9               # one vote cell: every other grid cell takes its winner
        huge = (np.uint32(0xFFFFFF00) + rng.randint(0, 256, size=votes.shape).astype(np.uint32)).astype(np.uint32)
        for grid in grids:
            _check_select(sd, votes, H, step, R, grid, "random counts")
            want = _check_select(sd, zeros, H, step, R, grid, "no votes")
            assert not want[0].any() and want[2] == 0
            want = _check_select(sd, hot, H, step, R, grid, "one hot cell")
            assert (want[0] == R).all() and int((want[1] != 0).sum()) == 1
            want = _check_select(sd, huge, H, step, R, grid, "counts near 2^32")
            assert shape == (1, 1) or int(want[3].max()) > 2 ** 32


# ---- the volume --------------------------------------------------------------------------------------------------------
def _field_volumes(sd, fl, fr, D, field, r, compare_offset=None):
    """The entry point inside an arena: features, field and both volumes at bases that are no multiple of 16, the volumes
    poisoned.  -> (left, right) [H,W,Dp] on the host after the red zones and the pads were found intact."""
    H, W, _ = fl.shape
    dp = sd.hwd_pitch(D)
    a = arena.Arena(2 * H * W * (dp + 64) * 4 + 12 * arena.GUARD, "cuda", fill="B")
    dfl, dfr = a.put(fl, base_mod16=4, name="fl"), a.put(fr, base_mod16=8, name="fr")
    dfield = a.put(np.ascontiguousarray(field, np.int32), base_mod16=4, name="field")
    left = a.take((H, W, dp), torch.float32, base_mod16=12, name="left", pads_from=D, output=True)
    right = a.take((H, W, dp), torch.float32, base_mod16=4, name="right", pads_from=D, output=True)
    a.poison()
    got = sd.cost_volume_field_hwd(dfl, dfr, D, dfield, r, out=(left, right))
    assert got[0] is left and got[1] is right
    a.check()
    for side, vol in (("left", left), ("right", right)):
        assert a.holds_fill(vol[..., D:]), "%s volume: a pad entry was written" % side
    if compare_offset is not None:                              # the shipped twin from the same run
        twin = sd.cost_volume_offset_hwd(dfl, dfr, D, torch.tensor([compare_offset], dtype=torch.int32, device="cuda"), r)
        for side in (0, 1):
            assert_bits(got[side][..., :D].cpu().numpy(), twin[side][..., :D].cpu().numpy(),
                        "constant field %d, range %d == mccnn_cost_volume_offset_hwd (%s)"
                        % (compare_offset, r, ("left", "right")[side]))
    return left.cpu().numpy(), right.cpu().numpy()


def _check_field(sd, fl, fr, D, field, r, what, compare_offset=None):
    got = _field_volumes(sd, fl, fr, D, field, r, compare_offset)
    want = vf.compute_cost_volume_field(fl, fr, D, field, r)
    for side in (0, 1):
        assert_bits(vr.hwd_to_dhw(got[side], D), want[side], "%s, range %d, %s volume" % (what, r, ("left", "right")[side]))
    return want


# H x W x D and a field of mixed signs on the grid where tile (63), block (64), band and image edges disagree
VOLUMES = [((7, 130, 21), [[2, -1, 0], [-3, 1, 4], [0, -2, 3]]),
           ((4, 200, 70), [[1, -2, 3, 0]]),                                   # right-view partners cross bands; D % 4 != 0
           ((9, 66, 64), [[-1, 2], [3, -4], [0, 1]]),                         # D = W - 2
           ((5, 257, 130), [[0, 2, -2, 5, -5], [1, 1, -7, 0, 3]])]


@pytest.mark.parametrize("shape,field", VOLUMES)
def test_field_volume_mixed_signs(sd, shape, field):
    H, W, D = shape
    fl, fr = _features(H, W)
    for r in (0, 1):
        _check_field(sd, fl, fr, D, np.array(field, np.int32), r, "%dx%dx%d, mixed signs" % shape)


@pytest.mark.parametrize("shape,field", VOLUMES)
def test_field_volume_constant_field_is_the_offset_volume(sd, shape, field):
    H, W, D = shape
    fl, fr = _features(H, W)
    grid = np.array(field).shape
    for k, r in ((2, 0), (-3, 1), (0, 1), (8, 0)):
        want = _check_field(sd, fl, fr, D, np.full(grid, k, np.int32), r, "%dx%dx%d, constant %d" % (shape + (k,)),
                            compare_offset=k)
        offset = vo.compute_cost_volume_offset(fl, fr, D, k, r)
        assert_bits(want[0], offset[0], "the restatements agree")
    _check_field(sd, fl, fr, D, np.full((1, 1), -2, np.int32), 1, "%dx%dx%d, 1 x 1 grid" % shape, compare_offset=-2)


def test_field_volume_clamped_words_and_the_nearest_row(sd):
    """+-8 at H = 4: no candidate row lies inside the image for most rows; words outside the clamp act as +-8."""
    H, W, D = 4, 200, 70
    fl, fr = _features(H, W)
    for r in (0, 1):
        _check_field(sd, fl, fr, D, np.array([[8, -8, 8, -8], [-8, 0, 8, 3]], np.int32), r, "4x200x70, +-8")
        want = _check_field(sd, fl, fr, D, np.array([[1000, INT32_MIN, 9, -9]], np.int32), r, "4x200x70, wild words")
        acts_as = vf.compute_cost_volume_field(fl, fr, D, np.array([[8, -8, 8, -8]], np.int32), r)
        assert_bits(want[0], acts_as[0], "wild words act as +-8")
    H, W, D = 7, 130, 21
    fl, fr = _features(H, W)
    _check_field(sd, fl, fr, D, np.array([[2 ** 31 - 1, -5, INT32_MIN], [7, 8, -8]], np.int32), 1, "7x130x21, wild words")


def test_field_volume_special_values(sd):
    H, W, D = 7, 130, 21
    field = np.array([[2, -1, 0], [-3, 1, 4], [0, -2, 3]], np.int32)
    nan = np.float32("nan")
    fl, fr = (a.copy() for a in _features(H, W, seed=41))
    fl[2, 70, :] = nan
    fr[4, 20, :] = nan
    fl[5, ::3, ::2] = -0.0
    fr[1, :, 1::2] = -0.0
    fl[6], fr[0] = 0.0, -0.0
    for r in (0, 1):
        want = _check_field(sd, fl, fr, D, field, r, "a NaN and a -0.0 feature vector")
        assert np.isnan(want[0][:, 2, 70]).all() and np.isnan(want[1][:, 4, 20]).all()
        assert not np.isnan(want[0][:, 0, D:]).any()


# ---- the matcher -------------------------------------------------------------------------------------------------------
PAIR = (40, 200, 16)
EXTRAS = dict(vertical_offset="grid", vertical_offset_grid=(2, 4), vertical_offset_max=4, vertical_offset_rows=2)


def _sheared_pair(H, W, D, seed, ax=2):
    """A synthetic pair whose right image is sheared by whole rows: (L, R) standardised [H,W,1], and their bytes."""
    import synthetic
    l8, r8, _ = synthetic.make_scene_u8(H, W, D, seed)
    r8 = vf.shear(r8, ax, 0)[0]
    return synthetic.standardize(l8), synthetic.standardize(r8), l8, r8


@pytest.fixture(scope="module")
def pair(sd, net):
    """The pair on the device, its features on the host, the restated measurement and volumes at ranges 0 and 1."""
    H, W, D = PAIR
    L, R, l8, r8 = _sheared_pair(H, W, D, seed=5)
    l, r = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    dfl, dfr = net.features_pair_hwc_split(l[:, :, 0].contiguous(), r[:, :, 0].contiguous())
    fl, fr = dfl.cpu().numpy(), dfr.cpu().numpy()
    votes = vo.vertical_profile(fl, fr, D, 4, 2)
    field, cells, offset, totals = vf.field_select(votes, H, 2, 4, 2, 4)
    want = {rng: vf.compute_cost_volume_field(fl, fr, D, field, rng) for rng in (0, 1)}
    return dict(L=L, R=R, l=l, r=r, l8=l8, r8=r8, fl=fl, fr=fr, dfl=dfl, dfr=dfr, votes=votes, field=field, cells=cells,
                offset=offset, totals=totals, want=want)


def _stages(sd, net, pair, extras, want, what, **kw):
    """match(keep=) of a matcher with `extras`: kept volumes == `want`, every later stage == the CPU chain."""
    import oracle as o
    H, W, D = PAIR
    m = sd.StereoMatcher(net, extras=extras, **kw)
    keep = {}
    out = m.match(pair["l"], pair["r"], D, keep=keep)
    out = (out[0] if isinstance(out, tuple) else out).cpu().numpy()
    assert m.features == "split_f16" and not m.features_saturated()
    assert_bits(keep["cv"][0].cpu().numpy(), want[0], what + ": kept left cost volume")
    assert_bits(keep["cv"][1].cpu().numpy(), want[1], what + ": kept right cost volume")
    d = stagewise(keep, pair["L"], pair["R"], D, o)
    assert first_differing_stage(d) is None, (what, d)
    left = out[0] if kw.get("views") == "both" else out
    assert_bits(left, keep["bilateral"].cpu().numpy(), what + ": the returned map is the last stage")
    return m, out


def _want_report(pair):
    R = 4
    shares = [[vo.share(pair["cells"][a, b], int(pair["field"][a, b]), R) if pair["cells"][a, b].any() else 0.0
               for b in range(4)] for a in range(2)]
    return dict(offset=pair["offset"], totals=[int(t) for t in pair["totals"]],
                share=vo.share(pair["totals"], pair["offset"], R), grid=[2, 4], offsets=pair["field"].tolist(),
                cell_totals=[[[int(v) for v in cell] for cell in row] for row in pair["cells"]], cell_shares=shares)


def test_the_sheared_pair_measures_a_field_the_single_offset_misses(pair):
    assert len(set(pair["field"].ravel().tolist())) > 1, pair["field"]
    assert pair["field"][0, 0] < 0 < pair["field"][0, 3], pair["field"]


def test_matcher_grid_eager_is_the_composition_of_the_public_calls(sd, net, pair):
    H, W, D = PAIR
    m, out = _stages(sd, net, pair, EXTRAS, pair["want"][0], "vertical_offset='grid'")
    assert m.vertical_grid(H, W) == (2, 4)
    assert m.vertical_report(H, W, D) == _want_report(pair)
    # stage by stage through the public calls
    votes = sd.vertical_profile(pair["dfl"], pair["dfr"], D, 4, 2)
    assert np.array_equal(votes.cpu().numpy().view(np.uint32), pair["votes"])
    field, cells, offset, totals = sd.vertical_field_select(votes, H, 2, 4, (2, 4))
    assert np.array_equal(field.cpu().numpy(), pair["field"]) and int(offset.cpu()[0]) == pair["offset"]
    assert np.array_equal(cells.cpu().numpy().view(np.uint64), pair["cells"])
    left, right = sd.cost_volume_field_hwd(pair["dfl"], pair["dfr"], D, field, 0)
    assert_bits(vr.hwd_to_dhw(left.cpu().numpy(), D), pair["want"][0][0], "composed left volume")
    assert_bits(vr.hwd_to_dhw(right.cpu().numpy(), D), pair["want"][0][1], "composed right volume")
    assert_bits(m.match(pair["l"], pair["r"], D).cpu().numpy(), out, "match without keep")
    assert_bits(m.match_u8(torch.from_numpy(pair["l8"]).cuda(), torch.from_numpy(pair["r8"]).cuda(), D).cpu().numpy(), out,
                "match_u8")
    auto = sd.StereoMatcher(net, extras=dict(vertical_offset="auto", vertical_offset_rows=2))
    assert not np.array_equal(auto.match(pair["l"], pair["r"], D).cpu().numpy(), out)
    assert sorted(auto.vertical_report(H, W, D)) == ["offset", "share", "totals"]


def test_matcher_grid_captured_and_replayed(sd, net, pair):
    H, W, D = PAIR
    eager = sd.StereoMatcher(net, extras=EXTRAS).match(pair["l"], pair["r"], D).cpu().numpy()
    g = sd.StereoMatcher(net, extras=EXTRAS)
    for what in ("capture", "replay", "second replay"):
        assert_bits(g.match_graph(pair["l"], pair["r"], D).cpu().numpy(), eager, "match_graph (%s)" % what)
        assert g.vertical_report(H, W, D) == _want_report(pair), what
    assert len(g._graphs) == 1


def test_matcher_grid_with_both_views_confidence_semi_dense_and_range(sd, net, pair):
    H, W, D = PAIR
    m, out = _stages(sd, net, pair, dict(EXTRAS, vertical_range=1), pair["want"][1], "grid, range 1")
    kw = dict(views="both", confidence=("lrc",), semi_dense="lr")
    full = sd.StereoMatcher(net, extras=dict(EXTRAS, vertical_range=1), **kw)
    eager = [t.cpu().numpy() for t in full.match(pair["l"], pair["r"], D)]
    assert eager[0].shape == (2, H, W) and len(eager) == 3
    assert_bits(eager[0][0], out, "views='both': the left map")
    g = sd.StereoMatcher(net, extras=dict(EXTRAS, vertical_range=1), **kw)
    for what in ("capture", "replay"):
        got = [t.cpu().numpy() for t in g.match_graph(pair["l"], pair["r"], D)]
        for k, name in enumerate(("maps", "confidence planes", "sparse maps")):
            assert_bits(got[k], eager[k], "captured, everything on (%s): %s" % (what, name))
    assert g.vertical_report(H, W, D) == _want_report(pair)


def test_matcher_defaults_change_nothing(sd, net, pair):
    H, W, D = PAIR
    plain = sd.StereoMatcher(net)
    spelt = sd.StereoMatcher(net, extras=dict(vertical_offset=0, vertical_offset_grid=(8, 8)))
    assert_bits(spelt.match(pair["l"], pair["r"], D).cpu().numpy(), plain.match(pair["l"], pair["r"], D).cpu().numpy(),
                "the extras at their defaults")
    assert not [k for k in spelt.workspace(H, W, D) if k.startswith("v_")]
    auto = sd.StereoMatcher(net, extras=dict(vertical_offset="auto"))
    auto.match(pair["l"], pair["r"], D)
    assert sorted(k for k in auto.workspace(H, W, D) if k.startswith("v_")) == ["v_offset", "v_totals", "v_votes"]
    grid = sd.StereoMatcher(net, extras=EXTRAS)
    ws = grid.workspace(H, W, D)
    assert sorted(k for k in ws if k.startswith("v_")) == ["v_cells", "v_field", "v_offset", "v_totals", "v_votes"]
    assert tuple(ws["v_field"].shape) == (2, 4) and tuple(ws["v_cells"].shape) == (2, 4, 9)


def test_process_functional_switch(sd):
    import process_functional as pf
    H, W, D = 16, 130, 12
    fl, fr = _features(H, W, seed=31)
    votes = vo.vertical_profile(fl, fr, D, 2, 1)
    field = vf.field_select(votes, H, 1, 2, 2, 3)[0]
    with module_setting(pf, "VERTICAL_OFFSET", "grid"), module_setting(pf, "VERTICAL_OFFSET_GRID", (2, 3)), \
            module_setting(pf, "VERTICAL_OFFSET_PROFILE", (2, 1)):
        got = pf.compute_cost_volume(fl, fr, D)
        with module_setting(pf, "COST_VOLUME_MODE", "mfma"):
            with pytest.raises(ValueError, match="'exact' only"):
                pf.compute_cost_volume(fl, fr, D)
    want = vf.compute_cost_volume_field(fl, fr, D, field, 0)
    assert got[0].shape == (D, H, W) and isinstance(got[0], np.ndarray)
    assert_bits(got[0], want[0], "left")
    assert_bits(got[1], want[1], "right")
    assert pf.VERTICAL_OFFSET == 0 and pf.VERTICAL_OFFSET_GRID == (3, 4)


# ---- match.py ----------------------------------------------------------------------------------------------------------
CLI_H, CLI_W, CLI_D = 40, 136, 16
RELS = ["trainingH/pairA", "trainingH/pairB", "trainingH/pairC"]


def _tree(root):
    from PIL import Image
    data, lst = root / "data", root / "list.txt"
    for i, rel in enumerate(RELS):
        _, _, l8, r8 = _sheared_pair(CLI_H, CLI_W, CLI_D, seed=70 + i, ax=(2, -2, 0)[i])
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
           "--data_dir", str(data), "--save_dir", str(root / "out"), "-t", tag, "-s", "0", "-e", "2", "--resume",
           os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    out = {}
    for rel in RELS:
        d = root / "out" / ("submit_%s" % tag) / rel
        out[rel] = dict((name, (d / name).read_bytes()) for name in sorted(os.listdir(str(d))) if name != "timeMCCNN.txt")
    return out


GRID = ["--vertical_offset", "grid", "--vertical_offset_grid", "2x8", "--vertical_offset_rows", "2"]
AUTO = ["--vertical_offset", "auto", "--vertical_offset_rows", "2"]


def test_match_cli_writes_the_same_files_in_all_three_loops(tmp_path):
    data, lst = _tree(tmp_path)
    written = dict((tag, _cli(tmp_path, data, lst, tag, extra)) for tag, extra in (
        ("g", GRID), ("gf", GRID + ["--pairs_in_flight", "2"]), ("gp", GRID + ["--pipeline"]), ("a", AUTO)))
    fields = []
    for rel in RELS:
        files = written["g"][rel]
        assert sorted(files) == ["disp0MCCNN.pfm", "verticalMCCNN.json"]
        record = json.loads(files["verticalMCCNN.json"].decode())
        assert sorted(record) == ["cell_shares", "cell_totals", "grid", "max_offset", "offset", "offsets", "row_step",
                                  "share", "totals"]
        assert record["grid"] == [2, 3] and (record["max_offset"], record["row_step"]) == (4, 2)      # 2x8 clamped: 3 blocks
        assert np.array(record["offsets"]).shape == (2, 3) and np.array(record["cell_totals"]).shape == (2, 3, 9)
        assert sum(record["totals"]) == (CLI_H // 2) * CLI_W == int(np.array(record["cell_totals"]).sum())
        assert np.array(record["cell_totals"]).sum(axis=(0, 1)).tolist() == record["totals"]
        fields.append(record["offsets"])
        assert written["gf"][rel] == files, "%s: --pairs_in_flight 2 wrote other files" % rel
        assert written["gp"][rel] == files, "%s: --pipeline wrote other files" % rel
        # without 'grid' the file of 'auto' keeps its keys, and so its bytes: the same global measurement, no new key
        auto = json.loads(written["a"][rel]["verticalMCCNN.json"].decode())
        assert sorted(auto) == ["max_offset", "offset", "row_step", "share", "totals"]
        assert auto == {k: record[k] for k in auto}
        assert written["a"][rel]["verticalMCCNN.json"] == (json.dumps(auto, sort_keys=True) + "\n").encode()
    assert fields[0] != fields[1], "the two sheared pairs measured the same field"
