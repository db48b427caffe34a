"""GPU: match.py --confidence mmn,lrc --evaluate on files, in the three list loops (flagless, --pairs_in_flight 2,
--pipeline), on a three-pair Middlebury tree and a two-pair KITTI tree at 48 x 64 x 16: the loops write the same bytes,
every confidence PFM read back is the matcher's plane, a run without --confidence keeps the bytes of every file it writes
(the JSON files: everything but the new keys), the sparsification entries are there, agree with the restatement and the
list means are the means of the pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import confidence_reference as ref
from conftest import GOLDEN_DIR, ROOT
from helpers import assert_bits

pytestmark = pytest.mark.gpu

H, W, D = 48, 64, 16
MEASURES = ("mmn", "lrc")
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
CALIB = ("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
         "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")
LOOPS = (("plain", []), ("two", ["--pairs_in_flight", "2"]), ("pipe", ["--pipeline"]))
KEYS = ["auc", "auc_optimal", "bad_rate", "n", "threshold"]


def _match(lst, data, out, n, extra):
    cmd = [sys.executable, os.path.join(SRC, "match.py"), "-g", "0", "--list_file", str(lst), "--resume", RESUME,
           "--data_dir", str(data), "--save_dir", str(out), "-t", "c", "-s", "0", "-e", str(n - 1)] + [str(a) for a in extra]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def _files(root):
    """{relative path: bytes} of everything a run wrote, the wall-clock files left out."""
    out = {}
    for dirpath, _dirs, names in os.walk(str(root)):
        for name in names:
            rel = os.path.relpath(os.path.join(dirpath, name), str(root))
            if name == "timeMCCNN.txt" or os.sep + "time" + os.sep in os.sep + rel:
                continue
            out[rel] = open(os.path.join(dirpath, name), "rb").read()
    return out


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    from PIL import Image
    import synthetic
    import util
    root = tmp_path_factory.mktemp("conf")
    mb, k15 = root / "mb" / "trainingC", root / "k15" / "training"
    for d in ("image_2", "image_3", "disp_occ_0", "disp_noc_0"):
        os.makedirs(str(k15 / d))
    truth = {"mb": [], "k15": []}
    for i in range(3):
        _, _, left, right, dmap = synthetic.make_pair(H, W, D, seed=500 + i)
        rng = np.random.default_rng(i)
        os.makedirs(str(mb / ("pair%d" % i)))
        for name, img in (("im0.png", left), ("im1.png", right)):
            Image.fromarray(img, mode="L").save(str(mb / ("pair%d" % i) / name))
        (mb / ("pair%d" % i) / "calib.txt").write_text(CALIB % (W, H, D, D))
        gt = np.asarray(dmap, np.float32).copy()
        gt[rng.random((H, W)) < 0.2] = np.inf
        util.writePfm(gt, str(mb / ("pair%d" % i) / "disp0GT.pfm"))
        truth["mb"].append(gt)
        if i < 2:
            name = "%06d_10.png" % i
            for view, img in (("image_2", left), ("image_3", right)):
                Image.fromarray(np.repeat(img[:, :, None], 3, axis=2), mode="RGB").save(str(k15 / view / name))
            code = np.clip(np.rint(np.asarray(dmap, np.float64) * 256), 1, 65535).astype(np.uint16)
            occ = np.where(rng.random((H, W)) < 0.4, code, 0).astype(np.uint16)
            util.write_png_u16(occ, str(k15 / "disp_occ_0" / name))
            util.write_png_u16(np.where(rng.random((H, W)) < 0.8, occ, 0).astype(np.uint16), str(k15 / "disp_noc_0" / name))
            truth["k15"].append(occ)
    (root / "mb.txt").write_text("".join("%s/im0.png\n" % (mb / ("pair%d" % i)) for i in range(3)))
    (root / "k15.txt").write_text("".join("%s\n" % (k15 / "image_2" / ("%06d_10.png" % i)) for i in range(2)))
    return dict(root=root, truth=truth)


@pytest.fixture(scope="module")
def runs(trees):
    root = trees["root"]
    conf = ["--confidence", "lrc,mmn", "--evaluate"]
    files = {}
    for name, extra in LOOPS:
        _match(root / "mb.txt", root / "mb", root / ("mb_" + name), 3, conf + extra)
        _match(root / "k15.txt", root / "k15", root / ("k15_" + name), 2,
               ["--dataset", "kitti2015", "--ndisp", D] + conf + extra)
    _match(root / "mb.txt", root / "mb", root / "mb_base", 3, ["--evaluate"])
    _match(root / "k15.txt", root / "k15", root / "k15_base", 2, ["--dataset", "kitti2015", "--ndisp", D, "--evaluate"])
    for tree in ("mb", "k15"):
        for name in ("plain", "two", "pipe", "base"):
            files[tree + "_" + name] = _files(root / ("%s_%s" % (tree, name)))
    return files


@pytest.fixture(scope="module")
def matcher(net_layers):
    import stereo_device as sd
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    return sd.StereoMatcher(net, confidence=MEASURES)


def _matched(matcher, left_path, right_path):
    import torch
    import util
    views = []
    for p in (left_path, right_path):
        g = util.read_gray(str(p)).astype(np.float32)
        views.append(torch.from_numpy(np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2)).cuda())
    disp, planes = matcher.match(views[0], views[1], D)
    return disp.cpu().numpy(), planes.cpu().numpy()


def _pfm(blob, tmp_path):
    import util
    p = tmp_path / "read.pfm"
    p.write_bytes(blob)
    return np.asarray(util.readPfm(str(p)), np.float32).reshape(H, W)


def _strip(obj):
    """A JSON file's content without the keys --confidence adds."""
    obj = json.loads(obj)
    obj.pop("sparsification", None)
    obj.get("mean", {}).pop("sparsification", None)
    for p in obj.get("pairs", []):
        p.pop("sparsification", None)
    return obj


@pytest.mark.parametrize("tree", ["mb", "k15"])
def test_three_loops_write_the_same_bytes_and_the_flag_changes_no_other_file(runs, tree):
    plain = runs[tree + "_plain"]
    conf_files = sorted(f for f in plain if "conf" in os.path.basename(f) or os.sep + "conf_" in os.sep + f)
    assert len(conf_files) == len(MEASURES) * (3 if tree == "mb" else 2), conf_files
    assert not any("msm" in f or "cur" in f for f in conf_files)
    for other in ("two", "pipe"):
        got = runs["%s_%s" % (tree, other)]
        assert sorted(got) == sorted(plain)
        for f in plain:
            assert got[f] == plain[f], "%s: %s differs from the flagless loop" % (other, f)
    base = runs[tree + "_base"]
    assert sorted(base) == sorted(f for f in plain if f not in conf_files)
    for f, blob in base.items():
        if f.endswith(".json"):
            assert _strip(plain[f]) == json.loads(blob), f
            assert b"sparsification" not in blob
        else:
            assert plain[f] == blob, "%s changed with --confidence" % f


def test_middlebury_planes_and_figures(trees, runs, matcher, tmp_path):
    root, plain = trees["root"], runs["mb_plain"]
    figures = []
    for i in range(3):
        pair = root / "mb" / "trainingC" / ("pair%d" % i)
        disp, planes = _matched(matcher, pair / "im0.png", pair / "im1.png")
        rel = os.path.join("submit_c", "trainingC", "pair%d" % i)
        assert_bits(_pfm(plain[os.path.join(rel, "disp0MCCNN.pfm")], tmp_path), disp, "pair %d map" % i)
        for k, name in enumerate(MEASURES):
            assert_bits(_pfm(plain[os.path.join(rel, "conf0MCCNN_%s.pfm" % name)], tmp_path), planes[k], "pair %d %s" % (i, name))
        s = json.loads(plain[os.path.join(rel, "evalMCCNN.json")])["sparsification"]
        assert sorted(s) == KEYS and sorted(s["auc"]) == sorted(MEASURES) and s["threshold"] == 1.0
        gt = trees["truth"]["mb"][i]
        region = np.isfinite(gt)
        with np.errstate(invalid="ignore"):
            bad = (~np.isfinite(disp) | (disp < 0) | (np.abs(disp - np.where(region, gt, np.float32(0))) > np.float32(1))) & region
        for k, name in enumerate(MEASURES):
            want = ref.sparsification(planes[k], bad, region)
            assert s["n"] == want["n"] and s["bad_rate"] == want["e"] / want["n"]
            assert abs(s["auc"][name] - want["auc"]) <= want["n"] * 2.0 ** -52
            assert abs(s["auc_optimal"] - want["auc_optimal"]) <= want["n"] * 2.0 ** -52
        figures.append(s)
    _check_list(json.loads(plain[os.path.join("submit_c", "eval.json")]), figures)


def _check_list(report, figures):
    assert [p["sparsification"] for p in report["pairs"]] == figures
    mean = report["mean"]["sparsification"]
    assert mean["pairs"] == len(figures) and mean["threshold"] == figures[0]["threshold"]
    for key in ("bad_rate", "auc_optimal"):
        assert mean[key] == sum(f[key] for f in figures) / len(figures)
    for name in MEASURES:
        assert mean["auc"][name] == sum(f["auc"][name] for f in figures) / len(figures)


def test_kitti_planes_and_figures(trees, runs, matcher, tmp_path):
    root, plain = trees["root"], runs["k15_plain"]
    figures = []
    for i in range(2):
        name = "%06d_10" % i
        _disp, planes = _matched(matcher, root / "k15" / "training" / "image_2" / (name + ".png"),
                                 root / "k15" / "training" / "image_3" / (name + ".png"))
        for k, measure in enumerate(MEASURES):
            blob = plain[os.path.join("submit_c", "conf_%s" % measure, name + ".pfm")]
            assert_bits(_pfm(blob, tmp_path), planes[k], "frame %d %s" % (i, measure))
        s = json.loads(plain[os.path.join("submit_c", "eval", name + ".json")])["sparsification"]
        assert sorted(s) == KEYS and sorted(s["auc"]) == sorted(MEASURES) and s["threshold"] == [3.0, 0.05]
        assert s["n"] == int((trees["truth"]["k15"][i] != 0).sum()) and 0.0 <= s["auc_optimal"] <= min(s["auc"].values())
        figures.append(s)
    _check_list(json.loads(plain[os.path.join("submit_c", "eval.json")]), figures)
