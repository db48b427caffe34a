"""GPU: match.py and train.py on synthetic KITTI trees, end to end on files.  The same images as a Middlebury tree give the
same maps - the same matcher, only the I/O differs - so the 16-bit PNGs decode to the encoded PFMs of the Middlebury run,
whichever of the three routes wrote them, and the evaluation files equal the restatement (tests/kitti_reference.py) on
what the PNGs hold."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import evaluation_reference as ref
import kitti_reference as kr
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu

D = 16
SIZES = [(40, 64), (40, 64), (38, 62)]         # two frames of one size (the second is captured with --pipeline), one of another
SRC = os.path.join(ROOT, "mc-cnn-python_amd", "src")
RESUME = os.path.join(GOLDEN_DIR, "mccnn_fast_weights.npz")
CALIB = ("cam0=[1 0 0; 0 1 0; 0 0 1]\ncam1=[1 0 0; 0 1 0; 0 0 1]\ndoffs=0\nbaseline=100\n"
         "width=%d\nheight=%d\nndisp=%d\nisint=0\nvmin=0\nvmax=%d\ndyavg=0\ndymax=0\n")


def _truth(dmap, seed):
    """Sparse 16-bit truth from the scene's disparity: about a third of the pixels in disp_occ, fewer in disp_noc, every
    known pixel's match inside the image (what the training pool asks of a pixel)."""
    rng = np.random.default_rng(seed)
    H, W = dmap.shape
    code = kr.encode(np.asarray(dmap, np.float32))
    code[(code // 256) > np.arange(W)[None, :]] = 0
    occ = np.where(rng.random((H, W)) < 0.35, code, 0).astype(np.uint16)
    noc = np.where(rng.random((H, W)) < 0.8, occ, 0).astype(np.uint16)
    return occ, noc


def _run(script, args):
    r = subprocess.run([sys.executable, os.path.join(SRC, script), "-g", "0"] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return r.stdout.decode()


def _match(lst, data, out, n, extra):
    return _run("match.py", ["--list_file", lst, "--resume", RESUME, "--data_dir", data, "--save_dir", out, "-t", "k",
                             "-s", "0", "-e", n - 1] + extra)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """The kitti2015 tree (colour PNGs), the same files as a Middlebury tree, and a kitti2012 pair with grey views."""
    from PIL import Image
    import synthetic
    import util
    root = tmp_path_factory.mktemp("kitti")
    k15, mb, k12 = root / "k15" / "training", root / "mb" / "trainingK", root / "k12" / "training"
    for d in ("image_2", "image_3", "disp_occ_0", "disp_noc_0"):
        os.makedirs(str(k15 / d))
    for d in ("image_0", "image_1", "disp_occ", "disp_noc"):
        os.makedirs(str(k12 / d))
    truth = []
    for i, (H, W) in enumerate(SIZES):
        _, _, left, right, dmap = synthetic.make_pair(H, W, D, seed=300 + i)
        name = "%06d_10.png" % i
        os.makedirs(str(mb / ("pair%d" % i)))
        for view, mb_name, img in (("image_2", "im0.png", left), ("image_3", "im1.png", right)):
            Image.fromarray(np.repeat(img[:, :, None], 3, axis=2), mode="RGB").save(str(k15 / view / name))
            shutil.copyfile(str(k15 / view / name), str(mb / ("pair%d" % i) / mb_name))
        (mb / ("pair%d" % i) / "calib.txt").write_text(CALIB % (W, H, D, D))
        occ, noc = _truth(dmap, seed=i)
        util.write_png_u16(occ, str(k15 / "disp_occ_0" / name))
        util.write_png_u16(noc, str(k15 / "disp_noc_0" / name))
        truth.append((occ, noc))
        if i == 0:
            for view, img in (("image_0", left), ("image_1", right)):
                Image.fromarray(img, mode="L").save(str(k12 / view / name))
            util.write_png_u16(occ, str(k12 / "disp_occ" / name))
            util.write_png_u16(noc, str(k12 / "disp_noc" / name))
    names = ["%06d_10" % i for i in range(len(SIZES))]
    (root / "k15.txt").write_text("".join("%s\n" % (k15 / "image_2" / (n + ".png")) for n in names))
    (root / "mb.txt").write_text("".join("%s/im0.png\n" % (mb / ("pair%d" % i)) for i in range(len(SIZES))))
    (root / "k12.txt").write_text("%s\n" % (k12 / "image_0" / (names[0] + ".png")))
    return dict(root=root, names=names, truth=truth)


@pytest.fixture(scope="module")
def runs(trees):
    root = trees["root"]
    n = len(SIZES)
    _match(root / "mb.txt", root / "mb", root / "out_mb", n, [])
    logs = {}
    for name, extra in (("plain", []), ("two", ["--pairs_in_flight", "2"]), ("pipe", ["--pipeline"])):
        logs[name] = _match(root / "k15.txt", root / "k15", root / ("out_" + name), n,
                            ["--dataset", "kitti2015", "--ndisp", D, "--evaluate"] + extra)
    return logs


def _pfm(trees, i):
    import util
    return np.asarray(util.readPfm(str(trees["root"] / "out_mb" / "submit_k" / "trainingK" / ("pair%d" % i) / "disp0MCCNN.pfm")),
                      np.float32)


def test_the_three_routes_write_the_same_png_and_it_is_the_encoded_middlebury_map(trees, runs):
    import util
    root = trees["root"]
    assert "pipeline: pairs=3 captures=1 replays=0 eager=2" in runs["pipe"]          # a new size is seen, not replayed
    for i, name in enumerate(trees["names"]):
        files = [(root / ("out_" + r) / "submit_k" / "disp_0" / (name + ".png")).read_bytes() for r in ("plain", "two", "pipe")]
        assert files[0] == files[1] == files[2] and len(files[0]) > 100, name
        code = util.read_u16(str(root / "out_plain" / "submit_k" / "disp_0" / (name + ".png")))
        pfm = _pfm(trees, i)
        assert code.shape == SIZES[i] == pfm.shape
        assert np.array_equal(code, kr.encode(pfm)), name
        assert (code != 0).mean() > 0.5
        for r in ("plain", "two", "pipe"):
            sub = root / ("out_" + r)
            assert float((sub / "submit_k" / "time" / (name + ".txt")).read_text()) > 0
            pgm = (sub / "submit_k_imgs" / "training" / "image_2" / (name + ".pgm")).read_bytes()
            assert pgm == (root / "out_plain" / "submit_k_imgs" / "training" / "image_2" / (name + ".pgm")).read_bytes()
            assert pgm.startswith(b"P5\n%d %d\n255\n" % (SIZES[i][1], SIZES[i][0]))


def test_evaluation_files_agree_across_routes_and_with_the_restatement(trees, runs):
    import util
    root = trees["root"]
    total = None
    per_pair = []
    for i, name in enumerate(trees["names"]):
        decoded = kr.decode(util.read_u16(str(root / "out_plain" / "submit_k" / "disp_0" / (name + ".png"))))
        want = kr.evaluate(decoded, trees["truth"][i][0], trees["truth"][i][1], kr.D1)
        per_pair.append(want)
        total = want if total is None else ref.accumulate(total, want)
        texts = [(root / ("out_" + r) / "submit_k" / "eval" / (name + ".json")).read_text() for r in ("plain", "two", "pipe")]
        assert texts[0] == texts[1] == texts[2]
        got = json.loads(texts[0])
        assert ref.same(got["raw"], want), (name, got["raw"], want)
        assert got["thresholds"] == [3.0] and got["rel_thresholds"] == [0.05] and got["interpolate"] is False
        a = want["all"]
        assert a["n_valid"] > 100 and got["all"]["bad"]["3.0"] == 100.0 * (a["n_bad"][0] + a["n_invalid"]) / a["n_valid"]
    lists = [json.loads((root / ("out_" + r) / "submit_k" / "eval.json").read_text()) for r in ("plain", "two", "pipe")]
    assert lists[0] == lists[1] == lists[2]
    zero = {name: dict(n_valid=0, n_invalid=0, n_bad=[0], sum_abs=0.0, sum_sq=0.0) for name in ref.REGIONS}
    assert ref.same(lists[0]["pooled"]["raw"], ref.accumulate(zero, total))
    assert [ref.same(p["raw"], w) for p, w in zip(lists[0]["pairs"], per_pair)] == [True] * 3
    assert lists[0]["skipped"] == [] and lists[0]["rel_thresholds"] == [0.05]


def test_eval_interpolate_scores_the_filled_map(trees, runs):
    import util
    root = trees["root"]
    _match(root / "k15.txt", root / "k15", root / "out_fill", 1,
           ["--dataset", "kitti2015", "--ndisp", D, "--evaluate", "--eval_interpolate", "--eval_thresholds", "3:0.05,1"])
    name = trees["names"][0]
    png = root / "out_fill" / "submit_k" / "disp_0" / (name + ".png")
    assert png.read_bytes() == (root / "out_plain" / "submit_k" / "disp_0" / (name + ".png")).read_bytes()
    want = kr.evaluate(kr.decode(util.read_u16(str(png))), trees["truth"][0][0], trees["truth"][0][1], ((3.0, 0.05), (1.0, 0.0)),
                       interpolate=True)
    got = json.loads((root / "out_fill" / "submit_k" / "eval" / (name + ".json")).read_text())
    assert ref.same(got["raw"], want) and got["interpolate"] is True and got["rel_thresholds"] == [0.05, 0.0]
    assert want["all"]["n_invalid"] == 0


def test_kitti2012_pair_with_grey_views(trees, runs):
    import util
    root = trees["root"]
    _match(root / "k12.txt", root / "k12", root / "out_k12", 1, ["--dataset", "kitti2012", "--ndisp", D, "--evaluate"])
    name = trees["names"][0]
    png = root / "out_k12" / "submit_k" / (name + ".png")
    code = util.read_u16(str(png))
    # grey views decode to the grey values the colour files of the 2015 tree convert to: the same map
    assert np.array_equal(code, kr.encode(_pfm(trees, 0)))
    assert (root / "out_k12" / "submit_k" / "time" / (name + ".txt")).is_file()
    assert (root / "out_k12" / "submit_k_imgs" / "training" / "image_0" / (name + ".pgm")).is_file()
    thr = tuple((t, 0.0) for t in (2.0, 3.0, 4.0, 5.0))
    want = kr.evaluate(kr.decode(code), trees["truth"][0][0], trees["truth"][0][1], thr)
    got = json.loads((root / "out_k12" / "submit_k" / "eval" / (name + ".json")).read_text())
    assert ref.same(got["raw"], want) and got["thresholds"] == [2.0, 3.0, 4.0, 5.0]
    assert ref.same(json.loads((root / "out_k12" / "submit_k" / "eval.json").read_text())["pooled"]["raw"], want)


def test_train_on_the_kitti_tree(trees, tmp_path):
    root = trees["root"]
    lists = tmp_path / "lists"
    lists.mkdir()
    for name in ("train.txt", "val.txt"):
        shutil.copyfile(str(root / "k15.txt"), str(lists / name))
    tb, ck = tmp_path / "tb", tmp_path / "ck"
    text = _run("train.py", ["--list_dir", lists, "--tensorboard_dir", tb, "--checkpoint_dir", ck, "--end_epoch", "2", "-bs",
                             "32", "--dataset", "kitti2015", "--ndisp", D, "--sampler", "device", "--sampling", "pool",
                             "--val_error", "--save_best", "--print_freq", "1"])
    n_valid = sum(int(np.count_nonzero(noc)) for _occ, noc in trees["truth"])
    assert "from a pool of %d pixels" % n_valid in text, text[-2000:]
    points = [json.loads(line) for line in (tb / "scalars.jsonl").read_text().splitlines()]
    for tag in ("val_d1_all", "val_d1_nonocc", "val_avgerr_all"):
        values = [p["value"] for p in points if p["tag"] == tag]
        assert len(values) == 2 and all(np.isfinite(v) for v in values), (tag, points)
    assert not [p for p in points if p["tag"].startswith("val_bad")]
    assert (ck / "model_best.ckpt.npz").is_file() and (ck / "model_epoch2.ckpt.npz").is_file()
    d1 = [p["value"] for p in points if p["tag"] == "val_d1_all"]
    best = min((1, 2), key=lambda e: (d1[e - 1], e))
    a, b = np.load(str(ck / "model_best.ckpt.npz")), np.load(str(ck / ("model_epoch%d.ckpt.npz" % best)))
    assert all(np.array_equal(a[k], b[k]) for k in b.files if "Momentum" not in k)


def test_middlebury_runs_do_not_change_with_the_flag_spelt_out(tmp_path):
    """The inputs of tests/test_evaluate_cli_gpu.py (40 x 64, 16 disparities, seeds 80 and 81, ground truth and mask):
    `--dataset middlebury` is the run without the flag, byte for byte, and the tree is the one match.py always wrote."""
    import test_evaluate_cli_gpu as mb
    data = tmp_path / "data"
    rels = ["trainingH/pairA", "trainingH/pairB"]
    for i, rel in enumerate(rels):
        mb._write_pair(str(data / rel), mb.H, mb.W, mb.D, seed=80 + i)
        mb._write_truth(str(data / rel), 1 + i, with_mask=i == 0)
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s/im0.png\n" % (data / rel) for rel in rels))
    _match(lst, data, tmp_path / "a", 2, ["--evaluate"])
    _match(lst, data, tmp_path / "b", 2, ["--evaluate", "--dataset", "middlebury", "--pipeline"])
    want = sorted(["submit_k/eval.json"] + ["submit_k/%s/%s" % (rel, f) for rel in rels
                                            for f in ("disp0MCCNN.pfm", "timeMCCNN.txt", "evalMCCNN.json")]
                  + ["submit_k_imgs/%s/disp0MCCNN.pgm" % rel for rel in rels])
    assert mb._tree(str(tmp_path / "a")) == want == mb._tree(str(tmp_path / "b"))
    for f in want:
        if not f.endswith("timeMCCNN.txt"):
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    got = json.loads((tmp_path / "a" / "submit_k" / rels[0] / "evalMCCNN.json").read_text())
    assert sorted(got) == ["all", "nonocc", "pair", "raw", "thresholds"] and got["thresholds"] == [0.5, 1.0, 2.0, 4.0]
    assert ref.same(got["raw"], mb._expected(data, rels[0], tmp_path / "a" / "submit_k" / rels[0] / "disp0MCCNN.pfm"))
