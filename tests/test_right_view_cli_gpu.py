"""GPU: match.py --views both on files, in the three list loops (flagless, --pairs_in_flight 2, --pipeline), on a
three-pair Middlebury tree at 48 x 64 x 16 with disp1GT.pfm on two of the pairs (mask1nocc.png on one): the loops write
the same bytes, the left files are those of a run without the flag, disp1MCCNN.pfm and conf1MCCNN_*.pfm read back are the
matcher's right map and planes, the "right" blocks equal evaluation_reference.evaluate on the written map, the pooled
right totals are the accumulation of the pairs', and the pair without disp1GT.pfm is skipped for the right view alone.
The KITTI layouts refuse the flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluation_reference as er
from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits

pytestmark = pytest.mark.gpu

H, W, D = 48, 64, 16
MEASURES = ("mmn", "lrc")
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
CALIB = ("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
         "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")
LOOPS = (("plain", []), ("two", ["--pairs_in_flight", "2"]), ("pipe", ["--pipeline"]))


def _run(lst, data, out, n, extra):
    cmd = [sys.executable, os.path.join(SRC, "match.py"), "-g", "0", "--list_file", str(lst), "--resume", RESUME,
           "--data_dir", str(data), "--save_dir", str(out), "-t", "v", "-s", "0", "-e", str(n - 1)] + [str(a) for a in extra]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)


def _files(root):
    out = {}
    for dirpath, _dirs, names in os.walk(str(root)):
        for name in names:
            if name != "timeMCCNN.txt":
                rel = os.path.relpath(os.path.join(dirpath, name), str(root))
                out[rel] = open(os.path.join(dirpath, name), "rb").read()
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from PIL import Image
    import synthetic
    import util
    root = tmp_path_factory.mktemp("views")
    mb = root / "mb" / "trainingV"
    truth = []
    for i in range(3):
        _, _, left, right, dmap = synthetic.make_pair(H, W, D, seed=700 + i)
        rng = np.random.default_rng(70 + i)
        pair = mb / ("pair%d" % i)
        os.makedirs(str(pair))
        for name, img in (("im0.png", left), ("im1.png", right)):
            Image.fromarray(img, mode="L").save(str(pair / name))
        (pair / "calib.txt").write_text(CALIB % (W, H, D, D))
        gt = np.asarray(dmap, np.float32).copy()
        gt[rng.random((H, W)) < 0.2] = np.inf
        util.writePfm(gt, str(pair / "disp0GT.pfm"))
        gt_r = mask_r = None
        if i < 2:                                    # the third pair has no right-view ground truth
            gt_r = np.roll(np.asarray(dmap, np.float32), -2, axis=1).copy()
            gt_r[rng.random((H, W)) < 0.25] = np.inf
            util.writePfm(gt_r, str(pair / "disp1GT.pfm"))
            if i == 0:
                mask_r = rng.choice(np.array([0, 128, 255], np.uint8), size=(H, W), p=[0.1, 0.2, 0.7])
                Image.fromarray(mask_r, mode="L").save(str(pair / "mask1nocc.png"))
        truth.append((gt, gt_r, mask_r))
    (root / "mb.txt").write_text("".join("%s/im0.png\n" % (mb / ("pair%d" % i)) for i in range(3)))
    return dict(root=root, truth=truth)


@pytest.fixture(scope="module")
def runs(tree):
    root = tree["root"]
    flags = ["--views", "both", "--confidence", "lrc,mmn", "--evaluate"]
    files = {}
    for name, extra in LOOPS:
        r = _run(root / "mb.txt", root / "mb", root / ("out_" + name), 3, flags + extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        files[name] = _files(root / ("out_" + name))
    r = _run(root / "mb.txt", root / "mb", root / "out_base", 3, ["--confidence", "lrc,mmn", "--evaluate"])
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    files["base"] = _files(root / "out_base")
    return files


def _is_right(rel):
    name = os.path.basename(rel)
    return name.startswith("disp1MCCNN") or name.startswith("conf1MCCNN")


def _strip(blob):
    obj = json.loads(blob)
    obj.pop("right", None)
    for p in obj.get("pairs", []):
        p.pop("right", None)
    return obj


def test_three_loops_write_the_same_bytes_and_the_left_files_keep_theirs(runs):
    plain = runs["plain"]
    right = sorted(f for f in plain if _is_right(f))
    assert len(right) == 3 * (2 + len(MEASURES)), right            # per pair: pfm, pgm, one plane per measure
    assert sum(f.endswith("disp1MCCNN.pgm") for f in right) == 3 and sum(f.endswith("disp1MCCNN.pfm") for f in right) == 3
    for other in ("two", "pipe"):
        got = runs[other]
        assert sorted(got) == sorted(plain)
        for f in plain:
            assert got[f] == plain[f], "%s: %s differs from the flagless loop" % (other, f)
    base = runs["base"]
    assert sorted(base) == sorted(f for f in plain if not _is_right(f))
    for f, blob in base.items():
        if f.endswith(".json"):
            assert _strip(plain[f]) == json.loads(blob), f
            assert b'"right"' not in blob
        else:
            assert plain[f] == blob, "%s changed with --views both" % f


def _pfm(blob, tmp_path):
    import util
    p = tmp_path / "read.pfm"
    p.write_bytes(blob)
    return np.asarray(util.readPfm(str(p)), np.float32).reshape(H, W)


def test_right_files_and_blocks(tree, runs, net_layers, tmp_path):
    import torch
    import stereo_device as sd
    import util
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    matcher = sd.StereoMatcher(net, confidence=MEASURES, views="both")
    root, plain = tree["root"], runs["plain"]
    report = json.loads(plain[os.path.join("submit_v", "eval.json")])
    pooled = None
    blocks = []
    for i in range(3):
        pair = root / "mb" / "trainingV" / ("pair%d" % i)
        views = []
        for p in (pair / "im0.png", pair / "im1.png"):
            g = util.read_gray(str(p)).astype(np.float32)
            views.append(torch.from_numpy(np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2)).cuda())
        maps, planes = matcher.match(views[0], views[1], D)
        maps, planes = maps.cpu().numpy(), planes.cpu().numpy()
        rel = os.path.join("submit_v", "trainingV", "pair%d" % i)
        written = _pfm(plain[os.path.join(rel, "disp1MCCNN.pfm")], tmp_path)
        assert_bits(written, maps[1], "pair %d: disp1MCCNN.pfm" % i)
        assert_bits(_pfm(plain[os.path.join(rel, "disp0MCCNN.pfm")], tmp_path), maps[0], "pair %d: disp0MCCNN.pfm" % i)
        for k, name in enumerate(MEASURES):
            assert_bits(_pfm(plain[os.path.join(rel, "conf1MCCNN_%s.pfm" % name)], tmp_path), planes[1, k],
                        "pair %d: conf1MCCNN_%s.pfm" % (i, name))
            assert_bits(_pfm(plain[os.path.join(rel, "conf0MCCNN_%s.pfm" % name)], tmp_path), planes[0, k],
                        "pair %d: conf0MCCNN_%s.pfm" % (i, name))
        pgm = util.saveDisparity
        ref_pgm = tmp_path / "ref.pgm"
        pgm(maps[1], str(ref_pgm))
        assert plain[os.path.join("submit_v_imgs", "trainingV", "pair%d" % i, "disp1MCCNN.pgm")] == ref_pgm.read_bytes()
        entry = json.loads(plain[os.path.join(rel, "evalMCCNN.json")])
        _gt, gt_r, mask_r = tree["truth"][i]
        if gt_r is None:
            assert "right" not in entry and "right" not in report["pairs"][i]
            continue
        block = entry["right"]
        want = er.evaluate(written, gt_r, mask_r, THRESHOLDS)
        assert er.same(block["raw"], want), "pair %d: the right block's counts and sums" % i
        assert sorted(block) == sorted(["all", "nonocc", "raw", "sparsification"])
        assert sorted(block["all"]) == sorted(entry["all"]) and sorted(block["sparsification"]) == sorted(entry["sparsification"])
        assert sorted(block["sparsification"]["auc"]) == sorted(MEASURES)
        assert block["sparsification"]["n"] == want["all"]["n_valid"]
        assert report["pairs"][i]["right"] == block
        blocks.append(block)
        pooled = want if pooled is None else er.accumulate(pooled, want)
    right = report["right"]
    assert sorted(right) == ["mean", "pooled", "skipped"]
    assert er.same(right["pooled"]["raw"], pooled), "the pooled right totals"
    assert right["skipped"] == [str(root / "mb" / "trainingV" / "pair2" / "im0.png")]
    assert report["skipped"] == []
    for region in er.REGIONS:
        assert right["mean"][region]["avgerr"] == sum(b[region]["avgerr"] for b in blocks) / 2
        for tag in right["mean"][region]["bad"]:
            assert right["mean"][region]["bad"][tag] == sum(b[region]["bad"][tag] for b in blocks) / 2
    assert right["mean"]["sparsification"]["pairs"] == 2


def test_kitti_refuses_the_flag(tree):
    root = tree["root"]
    for dataset in ("kitti2012", "kitti2015"):
        r = _run(root / "mb.txt", root / "mb", root / "out_kitti", 3, ["--dataset", dataset, "--views", "both"])
        text = r.stdout.decode()
        assert r.returncode == 2, text[-2000:]
        assert "--views both is not available with --dataset %s" % dataset in text
        assert "neither right-view" in text and "submission slot" in text
    assert not os.path.exists(str(root / "out_kitti"))


def test_right_view_is_scored_where_the_left_one_is(tmp_path):
    """The documented restriction: a pair with disp1GT.pfm but no disp0GT.pfm is matched and written as usual and listed
    as skipped for both views, in the flagless loop and in the pipeline alike."""
    from PIL import Image
    import synthetic
    import util
    pair = tmp_path / "mb" / "trainingV" / "only_right"
    os.makedirs(str(pair))
    _, _, left, right, dmap = synthetic.make_pair(H, W, D, seed=710)
    for name, img in (("im0.png", left), ("im1.png", right)):
        Image.fromarray(img, mode="L").save(str(pair / name))
    (pair / "calib.txt").write_text(CALIB % (W, H, D, D))
    util.writePfm(np.asarray(dmap, np.float32), str(pair / "disp1GT.pfm"))
    (tmp_path / "mb.txt").write_text("%s/im0.png\n" % pair)
    written = {}
    for name, extra in (("plain", []), ("pipe", ["--pipeline"])):
        r = _run(tmp_path / "mb.txt", tmp_path / "mb", tmp_path / ("out_" + name), 1, ["--views", "both", "--evaluate"] + extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        files = _files(tmp_path / ("out_" + name))
        rel = os.path.join("submit_v", "trainingV", "only_right")
        assert os.path.join(rel, "disp1MCCNN.pfm") in files and os.path.join(rel, "disp0MCCNN.pfm") in files
        assert os.path.join(rel, "evalMCCNN.json") not in files
        report = json.loads(files[os.path.join("submit_v", "eval.json")])
        assert report["pairs"] == [] and report["skipped"] == [str(pair / "im0.png")]
        assert report["right"]["skipped"] == [str(pair / "im0.png")]
        assert report["right"]["pooled"]["raw"]["all"]["n_valid"] == 0
        written[name] = files
    assert written["plain"] == written["pipe"]
