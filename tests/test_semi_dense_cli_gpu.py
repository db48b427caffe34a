"""GPU: match.py --semi_dense on files, in the three list loops (flagless, --pairs_in_flight 2, --pipeline), on a two-pair
Middlebury tree at 48 x 64 x 16 with both views' ground truth: the loops write the same bytes, every other file is that
of a run without the flag, disp0MCCNN_s.pfm / disp1MCCNN_s.pfm read back are the matcher's sparse maps, and the
"semi_dense" blocks equal evaluation_reference.evaluate on the written sparse map."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluation_reference as er
import semi_dense_reference as ref
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

H, W, D = 48, 64, 16
RULE = "lr,mmn:0.5,speckle:6:1"
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
CALIB = ("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
         "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")
LOOPS = (("plain", []), ("two", ["--pairs_in_flight", "2"]), ("pipe", ["--pipeline"]))
BASE = ["--views", "both", "--confidence", "mmn", "--evaluate"]


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
    root = tmp_path_factory.mktemp("semi")
    mb = root / "mb" / "trainingS"
    truth = []
    for i in range(2):
        _, _, left, right, dmap = synthetic.make_pair(H, W, D, seed=900 + i)
        rng = np.random.default_rng(90 + i)
        pair = mb / ("pair%d" % i)
        os.makedirs(str(pair))
        for name, img in (("im0.png", left), ("im1.png", right)):
            Image.fromarray(img, mode="L").save(str(pair / name))
        (pair / "calib.txt").write_text(CALIB % (W, H, D, D))
        gt = np.asarray(dmap, np.float32).copy()
        gt[rng.random((H, W)) < 0.2] = np.inf
        util.writePfm(gt, str(pair / "disp0GT.pfm"))
        gt_r = np.roll(np.asarray(dmap, np.float32), -2, axis=1).copy()
        gt_r[rng.random((H, W)) < 0.25] = np.inf
        util.writePfm(gt_r, str(pair / "disp1GT.pfm"))
        mask = None
        if i == 0:
            mask = rng.choice(np.array([0, 128, 255], np.uint8), size=(H, W), p=[0.1, 0.2, 0.7])
            Image.fromarray(mask, mode="L").save(str(pair / "mask0nocc.png"))
        truth.append((gt, mask, gt_r))
    (root / "mb.txt").write_text("".join("%s/im0.png\n" % (mb / ("pair%d" % i)) for i in range(2)))
    return dict(root=root, truth=truth)


@pytest.fixture(scope="module")
def runs(tree):
    root = tree["root"]
    files = {}
    for name, extra in LOOPS:
        r = _run(root / "mb.txt", root / "mb", root / ("out_" + name), 2, BASE + ["--semi_dense", RULE] + extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        files[name] = _files(root / ("out_" + name))
    r = _run(root / "mb.txt", root / "mb", root / "out_base", 2, BASE)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    files["base"] = _files(root / "out_base")
    return files


def _is_sparse(rel):
    return os.path.basename(rel) in ("disp0MCCNN_s.pfm", "disp1MCCNN_s.pfm")


def _strip(obj):
    """The JSON object without any "semi_dense" key, at every depth."""
    if isinstance(obj, dict):
        return dict((k, _strip(v)) for k, v in obj.items() if k != "semi_dense")
    if isinstance(obj, list):
        return [_strip(v) for v in obj]
    return obj


def test_three_loops_write_the_same_bytes_and_the_other_files_keep_theirs(runs):
    plain = runs["plain"]
    sparse = sorted(f for f in plain if _is_sparse(f))
    assert len(sparse) == 4, sparse
    for other in ("two", "pipe"):
        got = runs[other]
        assert sorted(got) == sorted(plain)
        for f in plain:
            assert got[f] == plain[f], "%s: %s differs from the flagless loop" % (other, f)
    base = runs["base"]
    assert sorted(base) == sorted(f for f in plain if not _is_sparse(f))
    for f, blob in base.items():
        if f.endswith(".json"):
            assert b'"semi_dense"' in plain[f] and b'"semi_dense"' not in blob
            assert _strip(json.loads(plain[f])) == json.loads(blob), f
        else:
            assert plain[f] == blob, "%s changed with --semi_dense" % f


def _pfm(blob, tmp_path):
    import util
    p = tmp_path / "read.pfm"
    p.write_bytes(blob)
    return np.asarray(util.readPfm(str(p)), np.float32).reshape(H, W)


def _check_block(block, want, rule_text):
    assert er.same(block["raw"], want), "the block's counts and sums"
    assert block["rule"] == rule_text
    for region in er.REGIONS:
        raw = want[region]
        scored = raw["n_valid"] - raw["n_invalid"]
        assert block["density"][region] == (100.0 * scored / raw["n_valid"] if raw["n_valid"] else None)
        assert block["bad_of_scored"][region] == dict(
            (tag, 100.0 * b / scored if scored else None) for tag, b in zip(sorted(block["bad_of_scored"][region], key=float),
                                                                           raw["n_bad"]))
        assert block[region]["invalid"] == (100.0 * raw["n_invalid"] / raw["n_valid"] if raw["n_valid"] else None)


def test_sparse_files_and_blocks(tree, runs, net_layers, tmp_path):
    import torch
    import stereo_device as sd
    import util
    from model import NET
    net = NET(None, input_patch_size=11, batch_size=1, device="cuda").set_layers(net_layers)
    matcher = sd.StereoMatcher(net, confidence=("mmn",), views="both", semi_dense=RULE)
    rule_text = matcher.semi_dense.describe()
    root, plain = tree["root"], runs["plain"]
    report = json.loads(plain[os.path.join("submit_v", "eval.json")])
    pooled = [None, None]
    for i in range(2):
        pair = root / "mb" / "trainingS" / ("pair%d" % i)
        views = []
        for p in (pair / "im0.png", pair / "im1.png"):
            g = util.read_gray(str(p)).astype(np.float32)
            views.append(torch.from_numpy(np.expand_dims((g - np.mean(g, axis=(0, 1))) / np.std(g, axis=(0, 1)), 2)).cuda())
        keep = {}
        maps, planes, sparse = matcher.match(views[0], views[1], D, keep=keep)
        maps, planes, sparse = maps.cpu().numpy(), planes.cpu().numpy(), sparse.cpu().numpy()
        rel = os.path.join("submit_v", "trainingS", "pair%d" % i)
        entry = json.loads(plain[os.path.join(rel, "evalMCCNN.json")])
        gt, mask, gt_r = tree["truth"][i]
        for v, (suffix, truth, truth_mask) in enumerate((("", gt, mask), ("_right", gt_r, None))):
            written = _pfm(plain[os.path.join(rel, "disp%dMCCNN_s.pfm" % v)], tmp_path)
            assert np.array_equal(ref.bits(written), ref.bits(sparse[v])), "pair %d: disp%dMCCNN_s.pfm" % (i, v)
            dense = _pfm(plain[os.path.join(rel, "disp%dMCCNN.pfm" % v)], tmp_path)
            assert np.array_equal(ref.bits(dense), ref.bits(maps[v]))
            want_sparse = ref.semi_dense(dense, matcher.semi_dense, keep["status" + suffix].cpu().numpy(), planes[v], ("mmn",))
            assert np.array_equal(ref.bits(written), ref.bits(want_sparse)), "pair %d view %d: the restatement" % (i, v)
            assert 0 < ref.valid(written).sum() < H * W
            block = (entry if v == 0 else entry["right"])["semi_dense"]
            want = er.evaluate(written, truth, truth_mask, THRESHOLDS)
            _check_block(block, want, rule_text)
            assert (report["pairs"][i] if v == 0 else report["pairs"][i]["right"])["semi_dense"] == block
            pooled[v] = want if pooled[v] is None else er.accumulate(pooled[v], want)
    for v, totals in enumerate((report, report["right"])):
        semi = totals["semi_dense"]
        assert sorted(semi) == ["mean", "pooled", "rule"] and semi["rule"] == rule_text
        assert er.same(semi["pooled"]["raw"], pooled[v]), "the pooled totals of view %d" % v
        blocks = [(p if v == 0 else p["right"])["semi_dense"] for p in report["pairs"]]
        for region in er.REGIONS:
            assert semi["mean"]["density"][region] == sum(b["density"][region] for b in blocks) / 2
            assert semi["mean"][region]["invalid"] == sum(b[region]["invalid"] for b in blocks) / 2


def test_parser_errors(tree):
    root = tree["root"]
    for extra, text in ((["--semi_dense", "lr,mmn:1"], "which --confidence does not name"),
                        (["--semi_dense", "lr,lr"], "named twice"),
                        (["--semi_dense", ""], "empty"),
                        (["--semi_dense", "lr", "--dataset", "kitti2015"], "--semi_dense is not available with --dataset")):
        r = _run(root / "mb.txt", root / "mb", root / "out_refused", 2, extra)
        out = r.stdout.decode()
        assert r.returncode == 2 and text in out, out[-2000:]
    assert not os.path.exists(str(root / "out_refused"))
